// nms_tail_launch.h -- the DEFINITION of launch_tail (K3..K6 in one launch: tail_kernel, nms_kernels.h).  Included by the
// nms_tail_<source>.hip units alone, which instantiate it for one overlap source each (nms_layer.h).
#pragma once
#include <algorithm>
#include "nms_kernels.h"
#include "nms_layer.h"

// K3..K6 in one launch (masked groups); SRC/src: kFromMatrix (the matrix), kFromBoxes (the boxes), kFromRecords (src unused)
template <int SRC>
int gnms_internal_launch_tail(const gnms::LayerCall& c, const float* src, int64_t ld, int sym, int chain_cap) {
    using namespace gnms;
    const int B = c.B, N = c.N;
    const int P2 = c.P2 < 1024 ? 1024 : c.P2;
    const int fast = (fast_tail_enabled() && fast_tail_ok(N, c.P, sym, chain_cap)) ? 1 : 0;
    const size_t lds = tail_lds_bytes(N, P2, fast);
    GNMS_CHECK_ARG(sym != 3 || fast, "launch_tail: the in-launch symmetry check needs the fast tail");
    int rc;
    GNMS_DISPATCH_SORT(P2, {
        if ((rc = allow_lds(tail_kernel<E, SRC>, lds))) return rc;
        const int spw = leaders_chain_wgs(N, sym, chain_cap);
        // sym 3: symmetry checkers in front of the chain (one 16-wave workgroup per 128 pairs of 64 x 64 bit blocks: fewer, so that the chain workgroups behind them in the grid start sooner, at most the CUs the chain leaves)
        int nchk = 0;
        if (sym == 3) {
            const long nb = (N + 63) / 64, pairs = (long)B * nb * (nb + 1) / 2;
            const int room = gnms_device_cu_count() - B * (spw + fast);
            nchk = (int)std::min<long>(std::max(room, 8), (pairs + 127) / 128);
            if (nchk < 1) nchk = 1;
        }
        tail_kernel<E, SRC><<<nchk + B * (spw + fast), 1024, lds, c.st>>>(src, N, (long)ld, c.counts, c.P, c.ws, c.L, P2, c.prob, (long long*)c.valid, (long long*)c.invalid,
                                                                          c.nvalid, c.ninvalid, sym, B, spw, fast, nchk);
    });
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
