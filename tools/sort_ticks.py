"""Developer: phase ticks of the one-launch sorts of 2048 < N <= 4096 keys (timing build, GNMS_EXTRA_FLAGS=-DGNMS_TIMING): wave 0 and wave 15 of
workgroup 8 of image 0, per role, for sort_ranked_runs_kernel (route 2), sort_hist_rank_kernel by histogram (route 3) and its fallback
(route 3 with the cap at 0).  s_memtime ticks (2.3-2.4 per ns), mean over the calls; every tick drains the wave's memory operations first."""
import ctypes, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from groomed_nms_amd import _lib, synthetic
from groomed_nms_amd._lib import GnmsParams, ptr, check
lib = _lib.load()
B, N = 8, 4096
P = GnmsParams(); lib.gnms_default_params(ctypes.byref(P))
NAMES = {0: ["key build + loads", "run sort", "LDS write + barrier", "searches", "second barrier", "gathers + stores"],
         1: ["key build + loads + range", "histogram atomics + barrier", "scan + barriers", "scatter + barrier", "gathers + count in the bin", "stores"],
         2: ["key build + loads + range", "histogram atomics + barrier", "scan barrier + run sort", "LDS write + barrier", "searches", "second barrier", "gathers + stores"]}
for kind in ("uniform", "clustered"):
    b, s = synthetic.batch_2d(1000, B, N, kind)
    boxes, scores = torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda()
    nbytes = lib.gnms_workspace_bytes(B, N, ctypes.byref(P))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    n4 = (4 * N + 255) // 256 * 256
    off = 14 * n4 + 600 * 8                                      # xsol, behind the bit-matrix kernel's slots
    reps = 20
    for path, route, cap in ((0, 2, -1), (1, 3, 769), (2, 3, 0)):
        lib.gnms_profile_set_hist_cap(cap)
        for rep in range(reps + 2):
            if rep == 2:
                ws[off:off + 192 * 8].zero_()
            check(lib.gnms_profile_sorts(ptr(scores), ptr(boxes), B, N, None, route, None, None, None, None, None, None, None, ptr(ws), nbytes, None), "sorts")
            torch.cuda.synchronize()
        t = ws[off:off + 192 * 8].cpu().numpy().view(np.int64).reshape(3, 2, 2, 16)[path] / reps   # [role][wave 0 / 15][slot]
        for role in (0, 1):
            for w, wname in ((0, "wave 0"), (1, "wave 15")):
                row = t[role, w, 1:1 + len(NAMES[path])]
                print("%s path %d (%s) role %d %s | %s | total %.0f ticks = %.2f us at 2.4 / ns" % (
                    kind, path, ("ranked runs", "histogram", "fallback")[path], role, wname,
                    " | ".join("%s %.0f" % (n, v) for n, v in zip(NAMES[path], row)), row.sum(), row.sum() / 2400.0), flush=True)
    lib.gnms_profile_set_hist_cap(-1)
