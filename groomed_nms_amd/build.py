"""Builds libgroomed_nms_hip.so (gfx950) in-tree with hipcc, and the C++ torch binding gnms_torch*.so (host compiler, links the
former).  `python -m groomed_nms_amd.build`."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libgroomed_nms_hip.so")
# Longest compile first (LABNOTES R15): the jobs start in this order, so the NMS layer's units -- 15 to 30 s each, everything else under 6 s -- go
# ahead of the small sources and a clean build takes about as long as the slowest of them.
SOURCES = ["nms_layer.hip", "nms_tail_write_records.hip", "nms_tail_write_boxes.hip", "nms_tail_boxes.hip", "nms_tail_matrix.hip", "nms_tail_records.hip",
           "soft_sort.hip", "aploss.hip", "iou_kernels.hip", "classic_nms.hip", "nms_profile.hip", "nms_others.hip", "proposals.hip", "host_mailbox.hip", "iou3d_exact.hip", "targets.hip", "detect3d.hip", "kitti_eval.hip", "kitti_rows.hip", "sampling.hip", "regression.hip", "after_nms.hip", "heads.hip", "loss.hip", "bbox_stats.hip", "preprocess.hip", "optim.hip", "iou_backward.hip", "iou3d_backward.hip"]
# -ffp-contract=off: products and sums round separately, like the reference's torch CPU kernels
# (lib/core.py:499-508) -- this is what makes the overlap matrices bit-identical.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-Wall", "-Werror=unused-function"] + os.environ.get("GNMS_EXTRA_FLAGS", "").split()      # (developer experiments: -DGNMS_TIMING ...)


def hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _depfile_deps(path):
    """The prerequisites in a make-style dependency file (hipcc -MD -MF), or None where it cannot be read."""
    try:
        text = open(path).read()
    except OSError:
        return None
    return text.replace("\\\n", " ").partition(":")[2].split()


def _jobs():
    """MAX_JOBS if set, else 8; never above 16."""
    try:
        n = int(os.environ.get("MAX_JOBS", ""))
    except ValueError:
        n = 8
    return max(1, min(n, 16))


def build(force=False, verbose=False):
    # objects compiled with other flags (GNMS_EXTRA_FLAGS experiments) are stale whatever else: the stamp is rewritten when the flags change
    # and every object depends on it
    stamp = os.path.join(CSRC, ".build_flags")
    flags = " ".join(FLAGS)
    if not os.path.exists(stamp) or open(stamp).read() != flags:
        with open(stamp, "w") as f:
            f.write(flags)
    objs, jobs = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace(".hip", ".o"))
        d = o[:-2] + ".d"                                    # what the compiler read for this object (-MD): the headers it really includes
        objs.append(o)
        deps = _depfile_deps(d)
        if force or deps is None or not all(os.path.exists(p) for p in deps) or _stale(o, [s, stamp, os.path.abspath(__file__)] + deps):
            jobs.append([hipcc()] + FLAGS + ["-MD", "-MF", d, "-c", s, "-o", o])
    if jobs:
        def run(cmd):
            if verbose:
                print(" ".join(cmd), flush=True)
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("hipcc failed:\n%s\n%s" % (" ".join(cmd), r.stderr[-6000:]))
            if verbose and r.stderr.strip():
                print(r.stderr[-3000:])
        with ThreadPoolExecutor(max_workers=_jobs()) as ex:                # (jobs start in SOURCES' order: longest first)
            list(ex.map(run, jobs))
    if jobs or force or _stale(OUT, objs):
        cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n%s" % r.stderr[-6000:])
    return OUT


TORCH_SRC = os.path.join(CSRC, "torch_binding.cpp")


def torch_binding_path():
    import sysconfig
    return os.path.join(HERE, "gnms_torch" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))


def build_torch_binding(force=False, verbose=False):
    """The C++ autograd binding (csrc/torch_binding.cpp): one host-compiler invocation against torch's headers, in-tree so that it
    travels to the GPU box like the HIP library it links (rpath $ORIGIN).  No device code, no GPU needed."""
    import sysconfig
    import torch
    from torch.utils import cpp_extension as ce
    out = torch_binding_path()
    lib = build()
    deps = [TORCH_SRC, os.path.join(HERE, "..", "include", "groomed_nms_hip.h"), os.path.abspath(__file__), lib]
    if not force and not _stale(out, deps):
        return out
    cxx = os.environ.get("CXX", "g++")
    inc = []
    for d in ce.include_paths(device_type="cuda") + [sysconfig.get_paths()["include"], os.path.join(os.environ.get("ROCM_HOME", "/opt/rocm"), "include")]:
        if d not in inc:
            inc.append(d)
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib")
    cmd = ([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-deprecated-declarations", "-Wno-unknown-pragmas",
            "-DTORCH_EXTENSION_NAME=gnms_torch", "-DTORCH_API_INCLUDE_EXTENSION_H", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
            "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI)]
           + ["-I" + d for d in inc] + [TORCH_SRC, "-o", out,
           "-L" + tlib, "-lc10", "-lc10_hip", "-ltorch_cpu", "-ltorch_hip", "-ltorch", "-ltorch_python",
           "-L" + HERE, "-lgroomed_nms_hip", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + tlib])
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("torch binding build failed:\n%s\n%s" % (" ".join(cmd), r.stderr[-8000:]))
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print(build_torch_binding(force="--force" in sys.argv, verbose=True))
