"""The KITTI object evaluation on the GPU: what the reference gets from 31 builds of data/kitti_split1/devkit/cpp/evaluate_object*.cpp
(lib/rpn_util.py:2043-2190, one subprocess per build), from one pass of HIP kernels (csrc/kitti_eval.hip, gnms_kitti_eval_*).

  load_results / load_labels      host parsers of the result / label folders (what the devkit's fscanf accepts) -> packed float64 rows
  evaluate                        rows + per-image offsets + variants -> precision [3 classes, 3 metrics, 3 difficulties, 41], aos, switches
  ap                              the means of parse_kitti_result (R40 / R11)
  write_stats                     stats_<cls>_detection.txt ... in saveStats' format (kitti_io.parse_kitti_result reads them)
  run_kitti_eval                  kitti_io.run_kitti_eval_script without the binary
  evaluate_kitti_results_verbose  lib/rpn_util.py:2076-2190: one load, one upload, one evaluate over all 30 variants
  evaluate_detections             the same dictionaries from a kitti_results.KittiResults (rows collected on the device) instead of a folder

A variant is (min_overlap [3 metrics][3 classes], max_depth or None): the two constants the devkit's sources differ in.  MAIN, SIDE and
DISTANCE_GRID[(metres, iou)] are the reference's 30.  There is no CPU implementation: the arithmetic runs in the kernels.  Limits:
MAX_DET detections and MAX_GT ground-truth rows per image; beyond them evaluate raises ValueError (nothing is truncated).

Row layouts (float64).  Detection: class id, alpha, x1 y1 x2 y2, h w l, t1 t2 t3, ry, score.  Ground truth: type id, truncation,
occlusion, alpha, x1 y1 x2 y2, h w l, t1 t2 t3, ry.  Ids: TYPE_IDS (a detection that is no Car / Pedestrian / Cyclist gets -1).
"""
import ctypes
import logging
import math
import os
import pickle

import numpy as np
import torch

from . import _lib
from .kitti_io import _cfg, parse_kitti_result

__all__ = ["MAIN", "SIDE", "DISTANCE_GRID", "CLASS_NAMES", "TYPE_IDS", "MAX_DET", "MAX_GT", "load_results", "load_labels", "evaluate", "ap",
           "write_stats", "run_kitti_eval", "evaluate_kitti_results_verbose", "evaluate_detections"]

CLASS_NAMES = ("car", "pedestrian", "cyclist")                       # evaluate_object.cpp:67-70
TYPE_IDS = {"car": 0, "pedestrian": 1, "cyclist": 2, "van": 3, "person_sitting": 4, "dontcare": 5}
OTHER_TYPE = 6
MAX_DET, MAX_GT = 512, 1024                                          # GNMS_KITTI_EVAL_MAX_DET / _MAX_GT
N_PTS = 41
DET_COLS, GT_COLS = 14, 15


def _variant(per_class, max_depth=None):
    return (tuple(tuple(float(x) for x in per_class) for _ in range(3)), max_depth)


MAIN = _variant((0.7, 0.5, 0.5))                                     # evaluate_object.cpp:61
SIDE = _variant((0.5, 0.3, 0.3))                                     # evaluate_object_0_5.cpp:61
# evaluate_object_<D>m_0_<k>.cpp: one value for all classes and metrics, `|| gt.t3 > D` in cleanData
DISTANCE_GRID = {(d, k / 10.0): _variant((k / 10.0,) * 3, float(d)) for d in (15, 30, 45, 60) for k in range(1, 8)}


# ---------------------------------------------------------------------------------------------------------------------------
# parsers
# ---------------------------------------------------------------------------------------------------------------------------
def _scan_double(tok):
    """what fscanf's %lf makes of a whole whitespace-delimited token, or None where the conversion fails"""
    try:
        return float(tok)
    except ValueError:
        return None


def _scan_int(tok):
    """%d: a decimal integer (a token like `1.00` would leave `.00` behind and derail the devkit's parse; such a line ends the file here)"""
    try:
        return float(int(tok, 10))
    except ValueError:
        return None


def _parse(text, n_fields, int_field, type_of):
    """the devkit's loop `while (!feof) if (fscanf(fmt) == n_fields) push`: the stream is a sequence of whitespace-separated tokens, a
    record is n_fields of them whatever the line breaks; a record the file ends in is dropped, and so is everything behind a token that
    does not convert (the devkit would resynchronise on some later token; files written by this project never have one)."""
    toks = text.split()
    rows = []
    for start in range(0, len(toks) - n_fields + 1, n_fields):
        rec = toks[start:start + n_fields]
        vals = [float(type_of(rec[0]))]
        for k in range(1, n_fields):
            v = _scan_int(rec[k]) if k == int_field else _scan_double(rec[k])
            if v is None:
                return rows
            vals.append(v)
        rows.append(vals)
    return rows


def _det_class(name):
    return {"car": 0, "pedestrian": 1, "cyclist": 2}.get(name.lower(), -1)      # strcasecmp, :180 / :459


def _gt_type(name):
    return TYPE_IDS.get(name.lower(), OTHER_TYPE)                                # strcasecmp, :414-451


def _pack(per_image, cols):
    offsets = np.zeros(len(per_image) + 1, np.int32)
    offsets[1:] = np.cumsum([len(r) for r in per_image])
    rows = np.array([r for img in per_image for r in img], np.float64).reshape(-1, cols)
    return rows, offsets


def _det_row(v):
    # file: type truncated occluded alpha x1 y1 x2 y2 h w l t1 t2 t3 ry score -> the two unused columns leave (:165-168)
    return [v[0]] + v[3:16]


def load_results(folder):
    """<folder>/*.txt in glob (sorted) order, as eval() reads them (:819).  Returns (det [n, 14], det_offsets [I + 1], names)."""
    names = sorted(f for f in os.listdir(folder) if f.endswith(".txt"))
    per_image = []
    for name in names:
        with open(os.path.join(folder, name)) as f:
            per_image.append([_det_row(v) for v in _parse(f.read(), 16, -1, _det_class)])
    det, offsets = _pack(per_image, DET_COLS)
    return det, offsets, names


def load_labels(folder, names):
    """the label files of the same names (:834).  Returns (gt [n, 15], gt_offsets [I + 1])."""
    per_image = []
    for name in names:
        with open(os.path.join(folder, name)) as f:
            per_image.append(_parse(f.read(), 15, 2, _gt_type))
    return _pack(per_image, GT_COLS)


# ---------------------------------------------------------------------------------------------------------------------------
# evaluate
# ---------------------------------------------------------------------------------------------------------------------------
def _host_offsets(off, what):
    if isinstance(off, torch.Tensor):
        off = off.detach().cpu().numpy()
    off = np.asarray(off)
    if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu":
        raise ValueError("%s must be a 1-D integer array of length I + 1" % what)
    if off.size and (int(off.max()) > np.iinfo(np.int32).max or int(off.min()) < 0):
        raise ValueError("%s out of the int32 range" % what)
    return np.ascontiguousarray(off, dtype=np.int32)


def _rows(x, cols, what, dev):
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1, cols)))
    if x.dim() != 2 or x.shape[1] != cols:
        raise ValueError("%s must be [n, %d]" % (what, cols))
    return x.to(device=dev, dtype=torch.float64).contiguous()


def _variant_arrays(variants):
    mins, depths = [], []
    for v in variants:
        m = np.asarray(v[0], np.float64)
        if m.shape != (3, 3):
            raise ValueError("a variant's min_overlap must be [3 metrics][3 classes]")
        mins.append(m)
        depths.append(math.inf if v[1] is None else float(v[1]))
    return np.stack(mins), np.asarray(depths, np.float64)


def evaluate(det, det_offsets, gt, gt_offsets, variants=(MAIN,), return_intermediates=False, device=None):
    """The devkit's eval() for every variant.  det [n, 14] / gt [m, 15] float64 rows (device tensors, or host arrays that are uploaded);
    det_offsets / gt_offsets [I + 1] int32 or int64, read on the host (they are the shapes of the ragged arrays).  Returns one dict per
    variant: precision [3 classes, 3 metrics, 3 difficulties, 41], aos [3, 3, 41] (NumPy float64; all 0 for a curve that is off),
    eval_image / eval_ground / eval_3d [3] bool, compute_aos bool; with return_intermediates also n_gt [3, 3, 3], thresholds
    [3, 3, 3, 41] with n_thresholds [3, 3, 3], tp / fp / fn [3, 3, 3, 41] and overlaps: per image [3 metrics, detections, ground
    truths], criterion -1 and on DontCare rows criterion 0.  The kernels are stream-ordered; the results are read once at the end."""
    variants = list(variants)
    if not variants:
        raise ValueError("evaluate needs at least one variant")
    lib = _lib.load()
    doff, goff = _host_offsets(det_offsets, "det_offsets"), _host_offsets(gt_offsets, "gt_offsets")
    if doff.size != goff.size:
        raise ValueError("det_offsets and gt_offsets describe %d and %d images" % (doff.size - 1, goff.size - 1))
    n_img, V = doff.size - 1, len(variants)
    n_pairs = ctypes.c_int64(0)
    if lib.gnms_kitti_eval_plan(doff.ctypes.data, goff.ctypes.data, n_img, V, ctypes.byref(n_pairs)) != 0:
        raise ValueError(lib.gnms_last_error().decode())
    n_pairs = n_pairs.value
    if device is None:
        device = det.device if isinstance(det, torch.Tensor) and det.is_cuda else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    det, gt = _rows(det, DET_COLS, "det", dev), _rows(gt, GT_COLS, "gt", dev)
    if det.shape[0] != int(doff[-1]) or gt.shape[0] != int(goff[-1]):
        raise ValueError("the offsets end at %d / %d, the arrays have %d / %d rows" % (doff[-1], goff[-1], det.shape[0], gt.shape[0]))
    n_det, n_gt_rows = det.shape[0], gt.shape[0]
    poff = np.zeros(n_img + 1, np.int64)
    poff[1:] = np.cumsum(np.diff(doff).astype(np.int64) * np.diff(goff).astype(np.int64))
    vmin, vdepth = _variant_arrays(variants)
    tasks = V * 27
    with _lib.on_device(dev):
        doff_d, goff_d, poff_d = (torch.from_numpy(a).to(dev) for a in (doff, goff, poff))
        vmin_d, vdepth_d = torch.from_numpy(vmin).to(dev), torch.from_numpy(vdepth).to(dev)
        i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
        overlaps = torch.empty((3, n_pairs), **f64)
        flags = torch.empty(10, **i32)
        tp_scores = torch.empty((tasks, n_gt_rows), **f64)
        n_tp, n_gt = torch.empty(tasks, **i32), torch.empty(tasks, **i32)
        st = _lib.stream_ptr(dev)
        _lib.check(lib.gnms_kitti_eval_recall(_lib.ptr(det), _lib.ptr(gt), _lib.ptr(doff_d), _lib.ptr(goff_d), _lib.ptr(poff_d), n_img, n_det,
                                              n_gt_rows, n_pairs, _lib.ptr(vmin_d), _lib.ptr(vdepth_d), V, _lib.ptr(overlaps), _lib.ptr(flags),
                                              _lib.ptr(tp_scores), _lib.ptr(n_tp), _lib.ptr(n_gt), st), "gnms_kitti_eval_recall")
        sorted_scores = torch.sort(tp_scores, dim=1, descending=True).values if n_gt_rows else tp_scores      # getThresholds' sort (:373)
        thresholds, n_thr = torch.empty((tasks, N_PTS), **f64), torch.empty(tasks, **i32)
        counts = torch.empty((tasks, N_PTS, 3), **i32)
        similarity = torch.empty((V, 9, n_img, N_PTS), **f64)
        precision, aos = torch.empty((tasks, N_PTS), **f64), torch.empty((V, 3, 3, N_PTS), **f64)
        _lib.check(lib.gnms_kitti_eval_precision(_lib.ptr(det), _lib.ptr(gt), _lib.ptr(doff_d), _lib.ptr(goff_d), _lib.ptr(poff_d), n_img, n_gt_rows,
                                                 n_pairs, _lib.ptr(vmin_d), _lib.ptr(vdepth_d), V, _lib.ptr(overlaps), _lib.ptr(flags),
                                                 _lib.ptr(sorted_scores), _lib.ptr(n_tp), _lib.ptr(n_gt), _lib.ptr(thresholds), _lib.ptr(n_thr),
                                                 _lib.ptr(counts), _lib.ptr(similarity), _lib.ptr(precision), _lib.ptr(aos), st),
                   "gnms_kitti_eval_precision")
        # the one host read
        precision_h = precision.cpu().numpy().reshape(V, 3, 3, 3, N_PTS)
        aos_h, flags_h = aos.cpu().numpy(), flags.cpu().numpy()
        if return_intermediates:
            n_gt_h = n_gt.cpu().numpy().reshape(V, 3, 3, 3)
            thr_h, n_thr_h = thresholds.cpu().numpy().reshape(V, 3, 3, 3, N_PTS), n_thr.cpu().numpy().reshape(V, 3, 3, 3)
            counts_h = counts.cpu().numpy().reshape(V, 3, 3, 3, N_PTS, 3)
            ov_h = overlaps.cpu().numpy()
            ov_list = []
            for i in range(n_img):
                nd, ng = int(doff[i + 1] - doff[i]), int(goff[i + 1] - goff[i])
                ov_list.append(ov_h[:, poff[i]:poff[i + 1]].reshape(3, ng, nd).transpose(0, 2, 1))
    out = []
    for v in range(V):
        r = {"precision": precision_h[v], "aos": aos_h[v], "compute_aos": not bool(flags_h[0]),
             "eval_image": flags_h[1:4].astype(bool), "eval_ground": flags_h[4:7].astype(bool), "eval_3d": flags_h[7:10].astype(bool)}
        if return_intermediates:
            r.update(n_gt=n_gt_h[v], thresholds=thr_h[v], n_thresholds=n_thr_h[v], tp=counts_h[v, ..., 0], fp=counts_h[v, ..., 1],
                     fn=counts_h[v, ..., 2], overlaps=ov_list)
        out.append(r)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's host tail
# ---------------------------------------------------------------------------------------------------------------------------
def ap(precision, use_40=True):
    """parse_kitti_result's means (lib/rpn_util.py:2031-2038) over the last axis: recall positions 1..40, or 0, 4, ..., 40."""
    p = np.asarray(precision, np.float64)
    sl = slice(1, 41, 1) if use_40 else slice(0, 41, 4)
    rows = p.reshape(-1, p.shape[-1])
    return np.array([np.mean(row[sl]) for row in rows]).reshape(p.shape[:-1])     # row by row: the reference's 1-D means, bit for bit


_FILES = (("det_2d_", "stats_{}_detection.txt", 0), ("or_", "stats_{}_orientation.txt", None), ("gr_", "stats_{}_detection_ground.txt", 1),
          ("det_3d_", "stats_{}_detection_3d.txt", 2))


def _curves(result, lbls):
    """(key prefix, file name, class name, [3 difficulties, 41]) of every curve that is on, in the devkit's order of writing"""
    for lbl in lbls:
        lbl = lbl.lower()
        if lbl not in CLASS_NAMES:
            continue
        c = CLASS_NAMES.index(lbl)
        on = (result["eval_image"][c], result["eval_image"][c] and result["compute_aos"], result["eval_ground"][c], result["eval_3d"][c])
        for (key, name, metric), use in zip(_FILES, on):
            if use:
                yield key, name.format(lbl), lbl, (result["aos"][c] if metric is None else result["precision"][c, metric])


def _stats_text(curve):
    return "".join("".join("%f " % x for x in row) + "\n" for row in curve)       # saveStats (:224-239)


def write_stats(result, folder, lbls=CLASS_NAMES):
    """the devkit's stats_<cls>_*.txt of one variant's result: three lines (easy, moderate, hard) of 41 `%f ` values.  Curves that
    are off get no file (and a stale one from an earlier run is removed, as the next parse would read it).  Returns the paths."""
    for lbl in lbls:
        for _, name, _ in _FILES:
            stale = os.path.join(folder, name.format(lbl.lower()))
            if os.path.exists(stale):
                os.remove(stale)
    paths = []
    for _, name, _, curve in _curves(result, lbls):
        paths.append(os.path.join(folder, name))
        with open(paths[-1], "w") as f:
            f.write(_stats_text(curve))
    return paths


def _results_dict(result, lbls, use_40):
    """what parse_kitti_result makes of the files write_stats would write, without writing them"""
    out = {}
    for key, _, lbl, curve in _curves(result, lbls):
        rounded = np.array([[float("%f" % x) for x in row] for row in curve])
        out[key + lbl] = list(ap(rounded, use_40=use_40))
    return out


def _load(results_data, gt_folder):
    det, doff, names = load_results(os.path.join(results_data, "data"))
    gt, goff = load_labels(gt_folder, names)
    return det, doff, gt, goff


def run_kitti_eval(results_data, gt_folder, lbls, variant=MAIN, use_40=True, write=True):
    """kitti_io.run_kitti_eval_script without the binary: reads <results_data>/data/*.txt and the labels of the same names, evaluates
    one variant, writes the stats files into results_data and returns {'det_2d_car': [easy, mod, hard], 'or_car': ..., ...}."""
    result = evaluate(*_load(results_data, gt_folder), variants=(variant,))[0]
    if not write:
        return _results_dict(result, lbls, use_40)
    out = {}
    written = set(write_stats(result, results_data, lbls))
    for lbl in lbls:
        lbl = lbl.lower()
        for key, name, _ in _FILES:
            path = os.path.join(results_data, name.format(lbl))
            if path in written:
                out[key + lbl] = list(parse_kitti_result(path, use_40=use_40))
    return out


def evaluate_detections(results, gt_folder, names, lbls, variants=(MAIN,), use_40=True):
    """run_kitti_eval / evaluate_kitti_results_verbose without the result folder: `results` is a kitti_results.KittiResults holding the
    split's detections on the device, `names` the label file of every appended image in order (`000001.txt`, ...).  Returns one
    {'det_2d_car': [easy, mod, hard], 'or_car': ..., ...} per variant (a list in the order of `variants`, or a dict with its keys when
    `variants` is a dict of name -> variant), built as parse_kitti_result would build them from the stats files."""
    keys = list(variants) if isinstance(variants, dict) else None
    vlist = [variants[k] for k in keys] if keys is not None else list(variants)
    gt, goff = load_labels(gt_folder, list(names))
    out = [_results_dict(r, lbls, use_40) for r in results.evaluate(gt, goff, variants=vlist)]
    return dict(zip(keys, out)) if keys is not None else out


def _report(results, lbls, test_iter, use_logging):
    for lbl in lbls:                                                              # lib/rpn_util.py:2110-2133
        lbl = lbl.lower()
        for task in ("det_2d", "or", "gr", "det_3d"):
            task_lbl = task + "_" + lbl
            if task_lbl in results:
                easy, mod, hard = results[task_lbl]
                task_print = task.replace("det_", "")
                if task_print == "gr":
                    task_print = "bev"
                print_str = "test_iter {} {} {:3s} --> easy: {:0.4f}, mod: {:0.4f}, hard: {:0.4f}".format(test_iter, lbl, task_print, easy, mod, hard)
                if use_logging:
                    logging.info(print_str)
                else:
                    print(print_str)


def evaluate_kitti_results_verbose(data_folder, test_dataset_name, results_folder, split_name="validation", test_iter=None, conf=None,
                                   use_logging=True, fast=False, default_eval="evaluate_object", write_pickle=True):
    """lib/rpn_util.py:2076-2190 with its printed / logged lines: main and side thresholds, then (unless `fast` or conf.fast_eval) the
    AP at 15 / 30 / 45 / 60 m x IoU 0.1 ... 0.7 -- one load, one upload and one evaluate over all variants instead of 30 subprocesses.
    Returns results_obj ({'main': ..., 'side': ..., 'res_15m_0_1': ...}); the reference returns None on the fast path and the full
    object nowhere -- it pickles it, which write_pickle does with the standard pickle module.  `default_eval` is accepted and unused
    (it names the binary).  The stats files left in the folder are the last variant's, as in the reference.  No plots."""
    stats_save_folder = os.path.dirname(results_folder)
    gt_folder = os.path.join(data_folder, test_dataset_name, split_name, "label_2")
    lbls = _cfg(conf, "lbls")
    is_fast = bool(fast or _cfg(conf, "fast_eval", False))
    iou_keys = ["0_1", "0_2", "0_3", "0_4", "0_5", "0_6", "0_7"]
    dis_keys = ["15", "30", "45", "60"]
    variants, names = [MAIN, SIDE], ["main", "side"]
    if not is_fast:
        for dis_key in dis_keys:
            for iou_key in iou_keys:
                variants.append(DISTANCE_GRID[(int(dis_key), int(iou_key[2:]) / 10.0)])
                names.append("res_{}m_{}".format(dis_key, iou_key))
    results = evaluate(*_load(stats_save_folder, gt_folder), variants=variants)
    write_stats(results[-1], stats_save_folder, lbls)
    results_obj = {name: _results_dict(r, lbls, True) for name, r in zip(names, results)}
    for name, title in (("main", "[0.7, 0.5, 0.5]"), ("side", "[0.5, 0.3, 0.3]")):
        print("")
        if use_logging:
            logging.info("Running for thresholds {}...".format(title))
        _report(results_obj[name], lbls, test_iter, use_logging)
    if is_fast:
        return results_obj
    for k, dis_key in enumerate(dis_keys):                                        # :2172-2188
        if k == 0:
            print("Getting AP3D at        ground truth distance <= {}m".format(dis_key), end="", flush=True)
        else:
            print("Getting AP3D at {}m <= ground truth distance <= {}m".format(dis_keys[k - 1], dis_key), end="", flush=True)
        for _ in iou_keys:
            print(".", end="", flush=True)
        print("", flush=True)
    if write_pickle:
        with open(os.path.join(stats_save_folder, "AP_vs_IOU3D_threshold_at_different_gt_distances.pkl"), "wb") as f:
            pickle.dump(results_obj, f)
    return results_obj
