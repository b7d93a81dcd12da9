"""Times the image front end (preprocess.preprocess_images, gnms_preprocess_images, csrc/preprocess.hip) at KITTI's size:
B = 2 images of 375 x 1242 x 3 uint8 -> float32 [2, 3, 512, 1760], the second one mirrored.
Before anything is timed the device result is compared with a float32 NumPy statement of the same operations at this size, bit for bit.
Reported, each the median and minimum of --iters repetitions after a warm-up:
  kernel_*        the launch alone from a device-resident buffer and table: HIP events around --burst back-to-back calls, divided by
                  the burst (a single launch of this size is shorter than the events' own cost), and the same replayed from a graph;
                  the algorithmic bytes (uint8 read once, float32 written once) over that time, beside a plain float4 store stream
                  (gnms_profile_fill) over the output's size timed the same way in the same process
  copy_*          the one pinned host-to-device copy of the packed batch (events)
  host_images_*   the whole call from host ndarrays: packing into the pinned buffer, copy, launch, synchronise (host clock)
  numpy_*         the NumPy statement on this machine's CPU, one thread of Python (host clock): what a user of the reference's loop
                  runs today, without cv2's resize, which NumPy stands in for
The script ends itself after --limit seconds.
usage: python tools/preprocess_time.py [--iters K] [--burst N] [--out FILE] [--no-numpy]  -> one JSON line."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from groomed_nms_amd import preprocess as P, _lib  # noqa: E402
from groomed_nms_amd._lib import check, ptr, stream_ptr  # noqa: E402

B, H, W = 2, 375, 1242
SIZE = [512, 1760]
MEANS, STDS = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
MIRROR = [False, True]
PEAK = 8.0e12
BYTES_IN = B * H * W * 3
BYTES_OUT = B * 3 * SIZE[0] * SIZE[1] * 4


def taps(n_dst, n_src):
    d = np.arange(n_dst, dtype=np.float64)
    s = ((d + 0.5) * (np.float64(n_src) / np.float64(n_dst)) - 0.5).astype(np.float32)
    fl = np.floor(s)
    f = (s - fl).astype(np.float32)
    i = fl.astype(np.int64)
    return np.clip(i, 0, n_src - 1), np.clip(i + 1, 0, n_src - 1), (np.float32(1) - f).astype(np.float32), f


def numpy_front_end(img, mirror):
    """lib/augmentations.py's Compose for one image in float32 NumPy, the bilinear resample in the place of cv2.resize, then the RGB
    swap and transpose of lib/imdb_util.py:522-526"""
    image = img.astype(np.float32)
    if mirror:
        image = np.ascontiguousarray(image[:, ::-1, :])
    scale_factor = SIZE[0] / image.shape[0]
    h = int(np.round(image.shape[0] * scale_factor))
    w = int(np.round(image.shape[1] * scale_factor))
    x0, x1, wx0, wx1 = taps(w, image.shape[1])
    y0, y1, wy0, wy1 = taps(h, image.shape[0])
    hor = image[:, x0, :] * wx0[None, :, None] + image[:, x1, :] * wx1[None, :, None]
    image = hor[y0] * wy0[:, None, None] + hor[y1] * wy1[:, None, None]
    if image.shape[1] > SIZE[1]:
        image = image[:, 0:SIZE[1], :]
    elif image.shape[1] < SIZE[1]:
        image = np.pad(image, [(0, 0), (0, SIZE[1] - image.shape[1]), (0, 0)], "constant")
    image /= 255.0
    image -= np.array(MEANS, np.float32)
    image /= np.array(STDS, np.float32)
    image[:, :, 0:3] = image[:, :, (2, 1, 0)]
    return np.ascontiguousarray(np.transpose(image, [2, 0, 1]))


def event_us(fn, iters, burst, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(burst):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / burst)
    return round(statistics.median(ts), 2), round(min(ts), 2)


def clock_us(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(ts), 1), round(min(ts), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the script ends itself")
    ap.add_argument("--no-numpy", action="store_true", help="skip the comparison with and the timing of the NumPy statement")
    args = ap.parse_args()
    signal.alarm(args.limit)
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
    table, nbytes, _, _ = P.describe([im.shape for im in images], SIZE, MIRROR)
    host = np.zeros((nbytes,), np.uint8)
    for im, row in zip(images, table):
        host[row[0]:row[0] + im.size] = im.reshape(-1)
    buffer, table_dev = torch.from_numpy(host).to(dev), torch.from_numpy(table).to(dev)
    line = dict(B=B, H=H, W=W, size=SIZE, iters=args.iters, burst=args.burst, MB_in=round(BYTES_IN / 1e6, 2), MB_out=round(BYTES_OUT / 1e6, 2))

    def kernel():
        return P.preprocess_images((buffer, table_dev), SIZE, MEANS, STDS)

    def from_host():
        out = P.preprocess_images(images, SIZE, MEANS, STDS, mirror=MIRROR)
        torch.cuda.synchronize()
        return out

    got = kernel()
    assert torch.equal(got, from_host()), "the host-image path and the device-buffer path differ"
    if not args.no_numpy:
        want = np.stack([numpy_front_end(im, m) for im, m in zip(images, MIRROR)])
        line["bit_identical_to_numpy_float32"] = bool(np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)))
        assert line["bit_identical_to_numpy_float32"], "the device result is not the float32 NumPy statement's"
        line["numpy_us"], line["numpy_min_us"] = clock_us(lambda: [numpy_front_end(im, m) for im, m in zip(images, MIRROR)], max(3, args.iters // 10), warm=1)

    # the launch alone
    line["kernel_us"], line["kernel_min_us"] = event_us(kernel, args.iters, args.burst)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            keep = kernel()
    torch.cuda.synchronize()
    line["kernel_graph_us"], line["kernel_graph_min_us"] = event_us(graph.replay, args.iters, args.burst)
    torch.cuda.synchronize()
    del keep, graph
    # a plain store stream over the output, timed the same way
    sink = torch.empty((BYTES_OUT // 4,), dtype=torch.float32, device=dev)
    sp = stream_ptr(dev)
    line["fill_us"], line["fill_min_us"] = event_us(lambda: check(lib.gnms_profile_fill(ptr(sink), sink.numel(), sp), "fill"), args.iters, args.burst)
    best = min(line["kernel_us"], line["kernel_graph_us"])
    line["kernel_TBs"] = round((BYTES_IN + BYTES_OUT) / (best * 1e-6) / 1e12, 3)
    line["kernel_fraction_of_8TBs"] = round((BYTES_IN + BYTES_OUT) / (best * 1e-6) / PEAK, 4)
    line["fill_TBs"] = round(BYTES_OUT / (line["fill_us"] * 1e-6) / 1e12, 3)
    line["kernel_store_rate_over_fill"] = round((BYTES_OUT / best) / (BYTES_OUT / line["fill_us"]), 3)

    # the pinned copy of the packed batch, and the whole call from host arrays
    pinned = torch.from_numpy(host).pin_memory()
    staged = torch.empty_like(buffer)
    line["copy_us"], line["copy_min_us"] = event_us(lambda: staged.copy_(pinned, non_blocking=True), args.iters, 1)
    line["copy_GBs"] = round(nbytes / (line["copy_us"] * 1e-6) / 1e9, 1)
    line["host_images_us"], line["host_images_min_us"] = clock_us(from_host, args.iters)
    if not args.no_numpy:
        line["numpy_over_host_images"] = round(line["numpy_us"] / line["host_images_us"], 1)
    torch.cuda.synchronize()
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
