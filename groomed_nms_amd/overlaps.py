"""Pairwise overlaps on MI355X -- mirror of the overlap helpers of the reference's lib/core.py and
lib/math_3d.py that feed the NMS.  Same names and argument meaning:
  iou(box_a, box_b, mode, data_type)                 lib/core.py:480-532
  intersect(box_a, box_b, mode, data_type)           lib/core.py:178-243
  iou3d_approximate(c1, c2, mode, method)            lib/core.py:305-421
  get_corners_of_cuboid(x, y, z, w, h, l, ry)        lib/math_3d.py:364-490
  iou3d(c1, c2, vol)                                 lib/core.py:246-302 (exact rotated IoU, csrc/iou3d_exact.hip)
  iou_ign(box_a, box_b, mode, data_type)             lib/core.py:535-575 (through gnms_compute_targets, csrc/targets.hip)
'combinations' mode runs in the HIP kernels (csrc/iou_kernels.hip); 'list' mode is O(N) elementwise
tensor arithmetic.  ndarray in -> ndarray out.  float64 ndarrays -- what the inference call site passes
(lib/rpn_util.py:1295: `aboxes` is float64 after the hstack at :1258) -- keep their dtype like the reference's
NumPy branches: `iou` (combinations) and `get_corners_of_cuboid` run the same IEEE double operations on the
GPU (gnms_iou2d_f64, gnms_corners_of_cuboid_f64), so the matrix that lib/groomed_nms.py:36 then rounds to
fp32 is the reference's bit for bit; other ndarrays are computed in fp32.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr, on_device
from .groomed_nms import _device

__all__ = ["iou", "intersect", "iou3d_approximate", "get_corners_of_cuboid", "iou_batched", "iou3d_batched", "iou3d",
           "iou3d_exact_batched", "iou_ign"]


def _is_f64_array(x):
    return isinstance(x, np.ndarray) and x.dtype == np.float64


def _to_dev(x, keep_grad=False):
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x)).to(device=_device(), dtype=torch.float32), "numpy", None
    dev = x.device if x.device.type == "cuda" else _device()
    if keep_grad and x.requires_grad and torch.is_grad_enabled():       # (iou: the moves are differentiable, the gradient flows back to `x`)
        return x.to(device=dev, dtype=torch.float32), "torch", x.device
    return x.detach().to(device=dev, dtype=torch.float32), "torch", x.device


def _back(t, kind, device):
    if kind == "numpy":
        return t.cpu().numpy()
    return t.to(device)


def _aligned(t):
    """`t` contiguous and 16-byte aligned (the kernels load a box as one float4): itself where it already is"""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _cotangent_layout(grad, B, M, N):
    """(tensor, ld) for a cotangent [B, M, N] of a RECTANGULAR overlap matrix as gnms_iou2d_backward reads it: unit column stride, row
    stride ld >= N, image stride M * ld.  A view that already lies so (a slice of a wider buffer) is used where it is; anything else
    (a transpose, an expanded tensor) is copied once.  (groomed_nms._matrix_layout is the square [B, N, N] form of this.)"""
    assert tuple(grad.shape) == (B, M, N)
    if B == 0 or M == 0 or N == 0:
        return grad.contiguous(), max(N, 1)
    ld = grad.stride(1)
    if grad.stride(2) == 1 and ld >= N and grad.stride(0) == M * ld:
        return grad, ld
    return grad.contiguous(), N          # (also where a size-1 dimension carries an arbitrary stride: the copy is then free)


def _pair_backward(ctx, grad, entry, *method):
    """(d_a, d_b) of an overlap matrix's cotangent `grad` [B, M, N]: the body of _Iou2dFunction.backward and _Iou3dFunction.backward.
    ctx saved (a, b), b None for a on both sides; `entry` names the library's backward (its workspace query is entry + "_workspace_bytes");
    `method` is gnms_iou3d_backward's extra argument."""
    a, b = ctx.saved_tensors
    lib = _lib.load()
    B, M, _ = a.shape
    N = M if b is None else b.shape[1]
    grad, ld = _cotangent_layout(grad.float(), B, M, N)
    d_a = torch.empty_like(a) if (b is None or ctx.needs_input_grad[0]) else None
    d_b = torch.empty_like(b) if (b is not None and ctx.needs_input_grad[1]) else None
    ws = torch.empty((max(getattr(lib, entry + "_workspace_bytes")(B, M, N), 256),), dtype=torch.uint8, device=a.device)
    with on_device(a.device):
        check(getattr(lib, entry)(ptr(a), ptr(b), ptr(grad), B, M, N, ld, *method, ptr(d_a), ptr(d_b), ptr(ws), ws.numel(),
                                  stream_ptr(a.device)), entry)
    return d_a, d_b


class _Iou2dFunction(torch.autograd.Function):
    """iou_batched with the gradient w.r.t. the boxes: the forward is the same gnms_iou2d launch, the backward is
    gnms_iou2d_backward (csrc/iou_backward.hip) -- the reference's iou() is a few torch operations that autograd differentiates
    (lib/core.py:499-508); this is that derivative in closed form.  boxes_b None: boxes_a on both sides."""

    @staticmethod
    def forward(ctx, boxes_a, boxes_b):
        a = _aligned(boxes_a)
        b = None if boxes_b is None else _aligned(boxes_b)
        ctx.save_for_backward(a, b)
        return iou_batched(a.detach(), None if b is None else b.detach())

    @staticmethod
    def backward(ctx, grad):
        return _pair_backward(ctx, grad, "gnms_iou2d_backward")


def iou_batched(boxes_a, boxes_b=None, out=None):
    """boxes_a [B,M,4], boxes_b [B,N,4] (CUDA fp32) -> [B,M,N].  boxes_b=None means boxes_a.  Differentiable w.r.t. the boxes: when
    one of them requires grad the result carries a grad_fn (gnms_iou2d_backward); otherwise it is a leaf, the same call as ever."""
    if torch.is_grad_enabled() and (boxes_a.requires_grad or (boxes_b is not None and boxes_b.requires_grad)):
        if out is not None:
            raise ValueError("iou_batched: `out` cannot be given when the boxes require grad")
        if not boxes_a.is_cuda or boxes_a.dtype != torch.float32 or (boxes_b is not None and boxes_b.dtype != torch.float32):
            raise TypeError("iou_batched: the gradient w.r.t. the boxes needs CUDA float32 boxes")
        return _Iou2dFunction.apply(boxes_a, None if boxes_b is boxes_a else boxes_b)
    from .groomed_nms import _binding
    ext = _binding()
    if ext and boxes_a.is_cuda and boxes_a.dtype == torch.float32 and (boxes_b is None or boxes_b.dtype == torch.float32):
        try:
            return ext.iou2d(boxes_a, boxes_a if boxes_b is None else boxes_b, out)
        except RuntimeError as e:                           # (the library's own failures only; torch's -- OOM first of all -- pass through)
            if isinstance(e, torch.cuda.OutOfMemoryError) or not str(e).startswith("GNMS:"):
                raise
            raise _lib.GnmsError(str(e)) from None
    lib = _lib.load()
    boxes_a = boxes_a.contiguous()
    boxes_b = boxes_a if boxes_b is None else boxes_b.contiguous()
    B, M, _ = boxes_a.shape
    N = boxes_b.shape[1]
    if out is None:
        out = torch.empty((B, M, N), dtype=torch.float32, device=boxes_a.device)
    with torch.cuda.device(boxes_a.device):
        check(lib.gnms_iou2d(ptr(boxes_a), ptr(boxes_b), B, M, N, ptr(out), N, stream_ptr(boxes_a.device)), "gnms_iou2d")
    return out


class _Iou3dFunction(torch.autograd.Function):
    """iou3d_batched(from_params=True) with the gradient w.r.t. the cuboids: the forward is the very call it makes without one, the
    backward is gnms_iou3d_backward (csrc/iou3d_backward.hip) -- the reference's get_corners_of_cuboid + iou3d_approximate are torch
    operations that autograd differentiates (lib/math_3d.py:364-435, lib/core.py:305-421); this is that derivative in closed form
    (DESIGN 3.24).  params_b None: params_a on both sides.  The second (BEV) output of want_bev is not differentiable."""

    @staticmethod
    def forward(ctx, params_a, params_b, method, want_bev, nms_overlap, nms_threshold):
        a = params_a.contiguous()
        b = None if params_b is None else params_b.contiguous()
        ctx.save_for_backward(a, b)
        ctx.method = 2 if nms_overlap else {"normal": 0, "generalized": 1}[method]
        res = iou3d_batched(a.detach(), None if b is None else b.detach(), method=method, from_params=True, want_bev=want_bev,
                            nms_overlap=nms_overlap, nms_threshold=nms_threshold)
        if want_bev:
            ctx.mark_non_differentiable(res[0])
        ctx.want_bev = want_bev
        return res

    @staticmethod
    def backward(ctx, *grads):
        grad = grads[-1]                                              # (bev, iou_3d) with want_bev: the matrix is the last output
        if grad is None:
            return (None,) * 6
        return _pair_backward(ctx, grad, "gnms_iou3d_backward", ctx.method) + (None,) * 4


def iou3d_batched(a, b=None, method="generalized", from_params=False, want_bev=False, nms_overlap=False, out=None, nms_threshold=None):
    """a [B,M,3,8] corners (or [B,M,7] params when from_params) -> iou_3d [B,M,N] (and iou_bev).
    nms_overlap=True returns 0.5*(1+giou), the matrix both reference callers hand to the NMS.  With nms_threshold (the threshold
    the layer will apply; square from-params problems) the HBM-bound kernel of gnms_nms_overlap3d_from_params writes it: within
    2e-6 of the exact operation order everywhere, and exactly that order wherever the threshold decision could depend on it.
    from_params=True is differentiable w.r.t. the cuboids: when one of them requires grad the result carries a grad_fn
    (gnms_iou3d_backward); otherwise it is a leaf, the same call as ever.  The corner form stays non-differentiable."""
    if from_params and torch.is_grad_enabled() and (a.requires_grad or (b is not None and b.requires_grad)):
        if out is not None:
            raise ValueError("iou3d_batched: `out` cannot be given when the cuboids require grad")
        if not a.is_cuda or a.dtype != torch.float32 or (b is not None and (b.dtype != torch.float32 or not b.is_cuda)):
            raise TypeError("iou3d_batched: the gradient w.r.t. the cuboids needs CUDA float32 parameters")
        if method not in ("normal", "generalized"):
            raise ValueError("unknown method {}".format(method))
        return _Iou3dFunction.apply(a, None if b is a else b, method, bool(want_bev), bool(nms_overlap), nms_threshold)
    lib = _lib.load()
    a = a.contiguous()
    if nms_overlap and from_params and b is None and nms_threshold is not None and not want_bev:
        B, N = a.shape[0], a.shape[1]
        o3 = out if out is not None else torch.empty((B, N, N), dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            check(lib.gnms_nms_overlap3d_from_params(ptr(a), B, N, float(nms_threshold), ptr(o3), max(N, 1), stream_ptr(a.device)),
                  "gnms_nms_overlap3d_from_params")
        return o3
    b = a if b is None else b.contiguous()
    B, M = a.shape[0], a.shape[1]
    N = b.shape[1]
    m = 2 if nms_overlap else {"normal": 0, "generalized": 1}[method]
    o3 = out if out is not None else torch.empty((B, M, N), dtype=torch.float32, device=a.device)
    bev = torch.empty((B, M, N), dtype=torch.float32, device=a.device) if want_bev else None
    fn = lib.gnms_iou3d_from_params if from_params else lib.gnms_iou3d_approximate
    with torch.cuda.device(a.device):
        check(fn(ptr(a), ptr(b), B, M, N, m, ptr(bev), ptr(o3), N, stream_ptr(a.device)), "gnms_iou3d")
    return (bev, o3) if want_bev else o3


def intersect(box_a, box_b, mode='combinations', data_type=None):
    """lib/core.py:178-243.  combinations -> N x M (note: [b][a], as in the reference); list -> M."""
    a, kind, dev = _to_dev(box_a)
    b, _, _ = _to_dev(box_b)
    if mode == 'combinations':
        max_xy = torch.min(a[:, 2:4], b[:, 2:4].unsqueeze(1))
        min_xy = torch.max(a[:, 0:2], b[:, 0:2].unsqueeze(1))
    elif mode == 'list':
        max_xy = torch.min(a[:, 2:4], b[:, 2:4])
        min_xy = torch.max(a[:, 0:2], b[:, 0:2])
    else:
        raise ValueError('unknown mode {}'.format(mode))
    inter = torch.clamp(max_xy - min_xy, 0)
    return _back(inter[..., 0] * inter[..., 1], kind, dev)


def iou(box_a, box_b, mode='combinations', data_type=None):
    """lib/core.py:480-532.  combinations: M x N matrix from the HIP kernel; list: M values."""
    if mode == 'combinations':
        # (both float64: with a float32 box_b the reference computes area_b in float32 before promoting -- that mix takes the fp32 kernel)
        if _is_f64_array(box_a) and _is_f64_array(box_b):
            # the reference's NumPy branch in float64 (lib/core.py:205-207, 512-513), the dtype its inference call site passes
            lib = _lib.load()
            dev = _device()
            a = torch.from_numpy(np.ascontiguousarray(box_a[:, :4], dtype=np.float64)).to(dev)
            b = torch.from_numpy(np.ascontiguousarray(box_b[:, :4], dtype=np.float64)).to(dev)
            M, N = a.shape[0], b.shape[0]
            out = torch.empty((M, N), dtype=torch.float64, device=dev)
            with on_device(dev):
                check(lib.gnms_iou2d_f64(ptr(a), ptr(b), 1, M, N, ptr(out), max(N, 1), stream_ptr(dev)), "gnms_iou2d_f64")
            return out.cpu().numpy()
        a, kind, dev = _to_dev(box_a, keep_grad=True)
        b = a if (box_b is box_a and a.requires_grad) else _to_dev(box_b, keep_grad=True)[0]
        av = a[:, :4].unsqueeze(0)
        # (iou(x, x) on one tensor: the same view on both sides, so that the gradient takes the one-box-set form of gnms_iou2d_backward)
        out = iou_batched(av, av if b is a else b[:, :4].unsqueeze(0))[0]
        return _back(out, kind, dev)
    if mode == 'list':
        # (torch arithmetic: differentiable w.r.t. the boxes like the reference's own expression)
        a, kind, dev = _to_dev(box_a, keep_grad=True)
        b, _, _ = _to_dev(box_b, keep_grad=True)
        max_xy = torch.min(a[:, 2:4], b[:, 2:4])
        min_xy = torch.max(a[:, 0:2], b[:, 0:2])
        wh = torch.clamp(max_xy - min_xy, 0)
        inter = wh[:, 0] * wh[:, 1]
        area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
        area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        return _back(inter / (area_a + area_b - inter), kind, dev)
    raise ValueError('unknown mode {}'.format(mode))


def get_corners_of_cuboid(x3d, y3d, z3d, w3d, h3d, l3d, ry3d, iou_3d_convention=True):
    """lib/math_3d.py:364-490, iou_3d_convention=True: the one every caller passes (lib/loss/rpn_3d.py:746-750, lib/rpn_util.py:1303).
    N x 3 x 8.  The reference's own iou_3d_convention=False branch is not usable: its torch form assigns an [N] tensor to an [N, 4]
    slice (math_3d.py:423-425: a shape error for every N but 1 and 4), its NumPy form has no such branch at all (:451-476: the box-frame
    corners stay zero) -- there is no behaviour to be faithful to, so it raises here."""
    if not iou_3d_convention:
        raise NotImplementedError("iou_3d_convention=False: the reference's own branch is broken (lib/math_3d.py:423-425 raises a shape error for "
                                  "N not in {1, 4}; the NumPy form lacks the branch); every caller passes True")
    lib = _lib.load()
    kind = "numpy" if isinstance(x3d, np.ndarray) else "torch"
    if kind == "numpy":
        # lib/math_3d.py:438-490: the NumPy branch builds R and the box-frame corners with .astype(float), i.e. in float64 whatever
        # the dtype of the arguments -- the corners come back as a float64 array
        dev = _device()
        params = torch.from_numpy(np.stack([np.asarray(v, dtype=np.float64).reshape(-1) for v in (x3d, y3d, z3d, w3d, h3d, l3d, ry3d)], 1)).to(dev)
        n = params.shape[0]
        corners = torch.empty((n, 3, 8), dtype=torch.float64, device=dev)
        with on_device(dev):
            # np.cos / np.sin evaluate in the dtype of ry3d (float32 at lib/rpn_util.py:1303-1309)
            trig_f32 = int(np.asarray(ry3d).dtype == np.float32)
            check(lib.gnms_corners_of_cuboid_f64(ptr(params), n, trig_f32, ptr(corners), stream_ptr(dev)), "gnms_corners_of_cuboid_f64")
        return corners.cpu().numpy()
    cols = [torch.as_tensor(v) for v in (x3d, y3d, z3d, w3d, h3d, l3d, ry3d)]
    out_device = cols[0].device
    dev = out_device if out_device.type == "cuda" else _device()
    params = torch.stack([c.to(device=dev, dtype=torch.float32).reshape(-1) for c in cols], dim=1).contiguous()
    n = params.shape[0]
    corners = torch.empty((n, 3, 8), dtype=torch.float32, device=dev)
    with on_device(dev):
        check(lib.gnms_corners_of_cuboid(ptr(params), n, ptr(corners), stream_ptr(dev)), "gnms_corners_of_cuboid")
    return _back(corners, kind, out_device)


def corners_batched(params):
    """params [B,N,7] (x, y, z, w, h, l, ry; CUDA fp32) -> corners [B,N,3,8]: get_corners_of_cuboid for a whole batch in one launch."""
    lib = _lib.load()
    params = params.contiguous()
    B, N = params.shape[0], params.shape[1]
    corners = torch.empty((B, N, 3, 8), dtype=torch.float32, device=params.device)
    with on_device(params.device):
        check(lib.gnms_corners_of_cuboid(ptr(params), B * N, ptr(corners), stream_ptr(params.device)), "gnms_corners_of_cuboid")
    return corners


def iou3d_approximate(corners_3d_b1, corners_3d_b2, mode="list", method="normal"):
    """lib/core.py:305-421.  Returns (iou_bev, iou_3d).  Inputs are NOT modified (the reference overwrites
    the y row of its inputs through a view, :379-380)."""
    c1, kind, dev = _to_dev(corners_3d_b1)
    c2, _, _ = _to_dev(corners_3d_b2)
    if c1.dim() == 2:
        c1, c2 = c1.unsqueeze(0), c2.unsqueeze(0)
    if method not in ("normal", "generalized"):
        raise ValueError("unknown method {}".format(method))
    if mode == "combinations":
        bev, i3 = iou3d_batched(c1.unsqueeze(0), c2.unsqueeze(0), method=method, want_bev=True)
        return _back(bev[0], kind, dev), _back(i3[0], kind, dev)
    if mode == "list":
        # O(N): the diagonal of the pairwise problem, done box by box on the same kernel
        n = c1.shape[0]
        bev, i3 = iou3d_batched(c1.reshape(n, 1, 3, 8), c2.reshape(n, 1, 3, 8), method=method, want_bev=True)
        return _back(bev.reshape(n), kind, dev), _back(i3.reshape(n), kind, dev)
    raise ValueError('unknown mode {}'.format(mode))


def iou3d_exact_batched(a, b=None, from_params=False, volume="box", want_bev=False, out=None):
    """The exact rotated IoU (lib/core.py:246-302) of every pair: a [B,M,3,8] corners (or [B,M,7] params when from_params), b likewise
    with N boxes (None: a) -> iou_3d [B,M,N], or (iou_bev, iou_3d) with want_bev.  CUDA fp32 in and out, float64 geometry inside.
    volume: "box" -- the sum of the boxes' own volumes (footprint area x height); "aabb" -- the sum of their corner AABB volumes, what
    the reference's iou3d uses when it is given no `vol` (:276-277)."""
    if volume not in ("box", "aabb"):
        raise ValueError("unknown volume {}".format(volume))
    lib = _lib.load()
    a = a.contiguous()
    b = a if b is None else b.contiguous()
    B, M = a.shape[0], a.shape[1]
    N = b.shape[1]
    o3 = out if out is not None else torch.empty((B, M, N), dtype=torch.float32, device=a.device)
    bev = torch.empty((B, M, N), dtype=torch.float32, device=a.device) if want_bev else None
    fn = lib.gnms_iou3d_exact_from_params if from_params else lib.gnms_iou3d_exact
    with on_device(a.device):
        check(fn(ptr(a), ptr(b), B, M, N, 0 if volume == "box" else 1, ptr(bev), ptr(o3), max(N, 1), stream_ptr(a.device)),
              "gnms_iou3d_exact")
    return (bev, o3) if want_bev else o3


def iou3d(corners_3d_b1, corners_3d_b2, vol=None):
    """lib/core.py:246-302: (iou_bev, iou_3d) of two cuboids given as (3, 8) corners -- two float64 scalars -- or of K pairs given as
    (K, 3, 8) arrays, with `vol` None, a scalar or (K,) -- two (K,) arrays.  vol None: the sum of the corner AABB volumes, as in the
    reference.  The footprints are intersected exactly in float64 on the GPU (gnms_iou3d_exact_list_f64) where the reference calls
    shapely.  Inputs are not modified.  ndarray in -> ndarray out; a torch tensor in -> a float64 tensor out on its device."""
    kind = "torch" if torch.is_tensor(corners_3d_b1) else "numpy"
    out_device = corners_3d_b1.device if kind == "torch" else None
    dev = out_device if kind == "torch" and out_device.type == "cuda" else _device()

    def dev64(x):
        if torch.is_tensor(x):
            return x.detach().to(device=dev, dtype=torch.float64).contiguous()
        return torch.from_numpy(np.array(x, dtype=np.float64)).to(dev)

    a, b = dev64(corners_3d_b1), dev64(corners_3d_b2)
    single = a.dim() == 2
    if single:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    if a.dim() != 3 or tuple(a.shape[1:]) != (3, 8) or a.shape != b.shape:
        raise ValueError("iou3d: corners must be (3, 8) or (K, 3, 8) and of the same shape, got %s and %s"
                         % (tuple(corners_3d_b1.shape), tuple(corners_3d_b2.shape)))
    k = a.shape[0]
    v = None if vol is None else dev64(vol).reshape(-1).expand(k).contiguous()
    bev = torch.empty(k, dtype=torch.float64, device=dev)
    i3 = torch.empty(k, dtype=torch.float64, device=dev)
    if k:
        lib = _lib.load()
        with on_device(dev):
            check(lib.gnms_iou3d_exact_list_f64(ptr(a), ptr(b), k, ptr(v), ptr(bev), ptr(i3), stream_ptr(dev)), "gnms_iou3d_exact_list_f64")
    if kind == "torch":
        bev, i3 = bev.to(out_device), i3.to(out_device)
        return (bev[0], i3[0]) if single else (bev, i3)
    bev, i3 = bev.cpu().numpy(), i3.cpu().numpy()
    return (np.float64(bev[0]), np.float64(i3[0])) if single else (bev, i3)


def iou_ign(box_a, box_b, mode='combinations', data_type=None):
    """lib/core.py:535-575: how much of each box_a lies inside each box_b, inter / (area_a + area_b * 0 - inter * 0), as [len(a), len(b)]
    float64.  NumPy combinations mode, the one compute_targets uses: box_b (the ignore regions) in float64, box_a in its own float32 /
    float64 for its area.  That is NumPy's result whenever either side is float64; two float32 inputs, which NumPy would keep in
    float32, are computed the same way (box_b widened) and come back as float64.  Runs the ignore pass of gnms_compute_targets."""
    if data_type is None:
        data_type = type(box_a)
    if mode != 'combinations':
        raise ValueError('unknown mode {}'.format(mode))
    if data_type is not np.ndarray:
        raise TypeError("iou_ign: NumPy arrays only (the reference's combinations mode on ndarrays)")
    from . import targets
    a = np.asarray(box_a)
    a = a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)
    b = np.asarray(box_b, dtype=np.float64).reshape(-1, 4)
    out = np.empty((a.shape[0], b.shape[0]), dtype=np.float64)
    if out.size == 0:
        return out
    dev = _device()
    ta = torch.from_numpy(np.ascontiguousarray(a[:, :4]))[None].to(dev)
    for k0 in range(0, b.shape[0], targets.MAX_GTS):
        tb = torch.from_numpy(np.ascontiguousarray(b[k0:k0 + targets.MAX_GTS]))[None].to(dev)
        t = targets.compute_targets_batched(ta, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, gts_ign=tb, want=("ols_ign",))
        out[:, k0:k0 + tb.shape[1]] = t.ols_ign[0].cpu().numpy()
    return out
