// nms_tail_write_launch.h -- tail_write_kernel (K3..K6 of every image + the matrix write in one launch) and the DEFINITION of its launcher.
// Included by the nms_tail_write_<source>.hip units alone, which instantiate the launcher for one overlap source each (nms_layer.h).
#pragma once
#include "gnms_prof.h"
#include "nms_kernels.h"
#include "nms_writers.h"
#include "nms_layer.h"

namespace {

using namespace gnms;

// chain_src: what the chain's single overlaps come from (the boxes for SRC = kFromBoxes; unused for kFromRecords: the workspace copy
// of the records); write_src: the writers' input (the boxes / the batch's contiguous records)
template <bool VEC, int E, int SRC>
__global__ __launch_bounds__(1024) void tail_write_kernel(const float* __restrict__ chain_src, const float* __restrict__ write_src, int N,
                                                          const int* __restrict__ counts, gnms_params P, char* ws, gnms_ws_layout L, int Ppow2,
                                                          float* __restrict__ prob, long long* __restrict__ valid,
                                                          long long* __restrict__ invalid, int* __restrict__ nvalid, int* __restrict__ ninvalid,
                                                          int nimg, float* __restrict__ out, long ld, int tile_rows, int row0, int row_end,
                                                          int staged, int fast) {
#ifdef GNMS_HWID    // developer experiment (tools/hwid_map.py): where the dispatcher put every workgroup of this launch
    if (threadIdx.x == 0) {
        unsigned* dbg = reinterpret_cast<unsigned*>(img_ptrs(ws, L, 0).rec);
        dbg[2 * blockIdx.x] = __builtin_amdgcn_s_getreg(63492);       // HW_ID
        dbg[2 * blockIdx.x + 1] = __builtin_amdgcn_s_getreg(63508);   // XCC_ID
    }
#endif
    const int spw = leaders_chain_wgs(N, 1);                          // scan workgroups per image (the from-boxes / from-records bit matrices are symmetric)
    const int cwg = spw + (fast ? 1 : 0);                             // + the fast tail's CSR workgroup (csr_build_body)
    if ((int)blockIdx.x < nimg * cwg) {
        int b;
        GNMS_TINIT();
#ifdef GNMS_TIMING
        long long tt__ = (long long)__builtin_amdgcn_s_memtime();
#define GNMS_TW_ACC(slot) do { long long n__ = (long long)__builtin_amdgcn_s_memtime(); if (threadIdx.x == 0 && b == 0) gnms::gnms_tbuf()[slot] += n__ - tt__; tt__ = n__; } while (0)
#else
#define GNMS_TW_ACC(slot) do {} while (0)
#endif
        if constexpr (E <= 4) {
            if (fast) {                                               // masked groups: leaders_sb_body<STAGE> -> fast_final_body ‖ csr_build_body
                if ((int)blockIdx.x >= nimg * spw) { csr_build_body<E>(N, counts, ws, L, (int)blockIdx.x - nimg * spw); return; }
                const int last = leaders_chain<SRC>(N, counts, ws, L, nimg, spw, (int)blockIdx.x, 1, &b, chain_src, (long)N, P.nms_threshold,
                                                    P.temperature, P.pruning_method, Ppow2);
                if (last) { GNMS_TW_ACC(5); fast_final_body<E, SRC>(chain_src, N, (long)N, counts, P, ws, L, Ppow2, prob, valid, invalid, nvalid, ninvalid, b, last); GNMS_TW_ACC(15); }
                GNMS_TFLUSH(ws, L, b);
                return;
            }
        }
        if (!leaders_chain(N, counts, ws, L, nimg, spw, (int)blockIdx.x, 1, &b)) return;   // (the image's other scan workgroups)
        __syncthreads();
        GNMS_TW_ACC(5);
        if (E <= 4 && P.mask_group_boxes) {                           // K4's rest rides in K5 (groups_body, FUSE), K6 starts from LDS
            if constexpr (E <= 4) {
                GNMS_TW_ACC(6);
                groups_body<E, SRC, true>(chain_src, N, (long)N, counts, P, ws, L, Ppow2, b);
                gnms::lds_barrier();
                GNMS_TW_ACC(7);
                finalize_body<E, true>(N, counts, P, ws, L, Ppow2, prob, valid, invalid, nvalid, ninvalid, b);
                GNMS_TW_ACC(15);
            }
            return;
        } else {
            attribute_image<SRC>(chain_src, (long)N, N, counts, P.nms_threshold, ws, L, b, 1);
            __syncthreads();
            GNMS_TW_ACC(6);
            groups_body<E, SRC>(chain_src, N, (long)N, counts, P, ws, L, Ppow2, b);
        }
        if (!P.mask_group_boxes) return;                              // unmasked groups: the solves (a launch of their own) come before K6
        __syncthreads();
        GNMS_TW_ACC(7);
        finalize_body<E>(N, counts, P, ws, L, Ppow2, prob, valid, invalid, nvalid, ninvalid, b);
        GNMS_TW_ACC(15);
        return;
    }
    const int first_writer = nimg * cwg;
    if (SRC == kFromBoxes && staged) { writers_staged_2d<VEC>(write_src, N, out, ld, nimg, img_ptrs(ws, L, 0).misc + 5, L.per_image / sizeof(int), first_writer); return; }
    if (SRC == kFromRecords && staged == 2) { writers_sym_persistent<true>(write_src, N, out, ld, nimg, P.nms_threshold, img_ptrs(ws, L, 0).misc + 5); return; }
    writers_persistent<VEC, SRC>(write_src, N, out, ld, nimg, tile_rows, row0, row_end, P.nms_threshold, img_ptrs(ws, L, 0).misc + 5);
}

// rows per wave tile of the write role: 16 measured best at B = 8, N = 4096 (0.168 ms per step; 8: 0.174, 32: 0.175, 64: 0.193 -- the last
// chunks of a launch end together only if chunks are short)
constexpr int kFusedTileRows = 16;

}  // namespace

// K3..K6 of every image + the matrix in one launch (tail_write_kernel)
template <int SRC>
int gnms_internal_launch_tail_write(const LayerCall& c, const float* chain_src, const float* write_src, float* out, int64_t ld) {
    const int B = c.B, N = c.N;
    const int P2 = c.P2 < 1024 ? 1024 : c.P2;
    const int fast = (fast_tail_enabled() && fast_tail_ok(N, c.P, 1)) ? 1 : 0;
    size_t lds = tail_lds_bytes(N, P2, fast);
    const int tr = kFusedTileRows;
    int staged = (SRC == kFromBoxes && N <= 4096) ? 1 : 0;           // writers_staged_2d: the image's boxes in LDS
    if (staged && lds < (size_t)N * 16) lds = (size_t)N * 16;
    long writers = write_chunk_count(N, B, tr, 0, N);                // persistent writers: at most one per CU
    if (SRC == kFromRecords && sym_writers_in_tail_launch(N, ld, out)) {   // writers_sym_persistent: two LDS macro tiles
        staged = 2;
        if (lds < 2 * gnms_iou3d::kSymTileBytes) lds = 2 * gnms_iou3d::kSymTileBytes;
        writers = (long)gnms_iou3d::sym_tiles_per_image(N) * B;
    }
    const int cus = gnms_device_cu_count();
    if (writers > cus) writers = cus;
    // How many CUs write.  With the packed row body (iou_tile.h) a writer workgroup sustains ~29 GB/s and the stream saturates near
    // 5.8 TB/s from ~200 of them; more writers add nothing to the matrix and slow the chain beside them, whose loads queue behind
    // the stores.  B = 8, N = 4096, same box, ms per step clustered / uniform: 216 writers 0.140 / 0.160, 208 0.139 / 0.158,
    // 200 0.140 / 0.151, 192 0.142 / 0.142, 184 0.144 / 0.144 -- at 24 writers per XCD the chain of the uniform images (1890
    // leaders each) stops being the longer side of the launch, at the price of 1.5 % on clustered ones.  (A plain fill in this
    // geometry: 6.2-6.4 TB/s from 64-128 workgroups, 5.8 from 248: profiles/r03*_store_geometry.jsonl.)
    const int cap = staged == 1 ? (cus * 208) / 256 : 0;
    if (cap > 0 && writers > cap) writers = cap;
    const dim3 grid((unsigned)(B * (leaders_chain_wgs(N, 1) + fast) + writers));
    const bool vec = (ld % 4 == 0) && ((uintptr_t)out % 16 == 0);
    int rc;
    GNMS_DISPATCH_SORT(P2, {
        if (vec) {
            if ((rc = allow_lds(tail_write_kernel<true, E, SRC>, lds))) return rc;
            gnms_launch_prof(kProfMatrixWrite, tail_write_kernel<true, E, SRC>, grid, dim3(1024), lds, c.st, chain_src, write_src, N, c.counts, c.P, c.ws,
                             c.L, P2, c.prob, (long long*)c.valid, (long long*)c.invalid, c.nvalid, c.ninvalid, B, out, (long)ld, tr, 0, N, staged, fast);
        } else {
            if ((rc = allow_lds(tail_write_kernel<false, E, SRC>, lds))) return rc;
            gnms_launch_prof(kProfMatrixWrite, tail_write_kernel<false, E, SRC>, grid, dim3(1024), lds, c.st, chain_src, write_src, N, c.counts, c.P,
                             c.ws, c.L, P2, c.prob, (long long*)c.valid, (long long*)c.invalid, c.nvalid, c.ninvalid, B, out, (long)ld, tr, 0, N, staged, fast);
        }
    });
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
