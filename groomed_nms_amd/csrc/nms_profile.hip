// nms_profile.hip -- the measurement entries of the C ABI (gnms_profile_*): the event pairs around the HBM-bound launches, the plain
// store / load streams the roofline is quoted beside, and the hooks that run one stage of the layer alone.  The stages themselves are
// nms_layer.hip's launchers (nms_layer.h): no kernel of the layer is compiled here.
#include <map>
#include <mutex>
#include <atomic>
#include <vector>
#include <algorithm>
#include "gnms_prof.h"
#include "nms_sort_kernels.h"
#include "nms_layer.h"

// ------------------------------------------------------------------------------------------------
// profiling: event pairs around the HBM-bound launches (bench.py's roofline is computed from these)
// ------------------------------------------------------------------------------------------------
namespace {
struct ProfPair { int dev; hipEvent_t start, stop; };
struct ProfState {
    std::atomic<bool> armed{false};
    std::mutex mu;
    std::map<int, std::vector<hipEvent_t>> pool;                   // recycled events, per device (an event belongs to the device it was created on)
    std::vector<ProfPair> pairs[kProfSlots];
    hipEvent_t take(int dev) {
        std::vector<hipEvent_t>& p = pool[dev];
        if (!p.empty()) { hipEvent_t e = p.back(); p.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
};
ProfState& prof() { static ProfState P; return P; }
}  // namespace

bool gnms_prof_armed() { return prof().armed.load(std::memory_order_relaxed); }
bool gnms_prof_pair(int slot, hipEvent_t* start, hipEvent_t* stop) {
    ProfState& P = prof();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lock(P.mu);
    hipEvent_t a = P.take(dev), b = P.take(dev);
    if (!a || !b) { if (a) P.pool[dev].push_back(a); if (b) P.pool[dev].push_back(b); return false; }
    P.pairs[slot].push_back(ProfPair{dev, a, b});
    *start = a;
    *stop = b;
    return true;
}

extern "C" int gnms_profile_events(int enable) {
    prof().armed.store(enable != 0, std::memory_order_relaxed);
    return GNMS_OK;
}

extern "C" int gnms_profile_collect(int slot, double* ms_sum, int* launches) {
    GNMS_CHECK_ARG(slot >= 0 && slot < kProfSlots && ms_sum && launches, "gnms_profile_collect: bad argument");
    ProfState& P = prof();
    std::lock_guard<std::mutex> lock(P.mu);
    double sum = 0.0;
    int n = 0;
    hipError_t first_err = hipSuccess;
    // every pair leaves the list and goes back to its device's pool whatever happens: an error on one pair is reported after the
    // walk, it never strands the others (or leaves recycled events behind in the list)
    for (const ProfPair& pr : P.pairs[slot]) {
        float ms = 0.0f;
        hipError_t e = hipEventSynchronize(pr.stop);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, pr.start, pr.stop);
        if (e == hipSuccess) { sum += ms; ++n; }
        else if (first_err == hipSuccess) first_err = e;
        P.pool[pr.dev].push_back(pr.start);
        P.pool[pr.dev].push_back(pr.stop);
    }
    P.pairs[slot].clear();
    *ms_sum = sum;
    *launches = n;
    if (first_err != hipSuccess) {
        gnms_set_error("gnms_profile_collect: %s", hipGetErrorString(first_err));
        return GNMS_ERR_HIP;
    }
    return GNMS_OK;
}

namespace {
// plain streams: what the HBM delivers to a kernel that does nothing else (the achievable ceiling the roofline is quoted beside)
__global__ __launch_bounds__(512) void prof_fill_kernel(float4* __restrict__ dst, size_t n4, float v) {
    const float4 x = make_float4(v, v, v, v);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float* p = reinterpret_cast<float*>(dst + i);
        __builtin_nontemporal_store(x.x, p); __builtin_nontemporal_store(x.y, p + 1);
        __builtin_nontemporal_store(x.z, p + 2); __builtin_nontemporal_store(x.w, p + 3);
    }
}
__global__ __launch_bounds__(512) void prof_read_kernel(const float4* __restrict__ src, size_t n4, float* __restrict__ sink) {
    float acc = 0.0f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float* p = reinterpret_cast<const float*>(src + i);
        acc += __builtin_nontemporal_load(p) + __builtin_nontemporal_load(p + 1) + __builtin_nontemporal_load(p + 2) + __builtin_nontemporal_load(p + 3);
    }
    if (acc == 123456.789f) *sink = acc;                          // never true for the data it is run on; keeps the loads alive
}
// the same bytes in the geometry of the matrix writers: a wave stores ROWS rows x 1 KiB (rows `ld` floats apart), 16 waves side by side,
// one workgroup per CU walking the row bands -- no loads, no arithmetic
template <int ROWS, bool NT>
__global__ __launch_bounds__(1024) void prof_fill_tiles_kernel(float* __restrict__ dst, int N, long ld, long bands, float v, int order) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncc = (N + 255) >> 8;
    const int ncg = (ncc + 15) >> 4;                              // column groups of 16 wave tiles (4096 columns)
    const long units = bands * ncg;
    const long bands_img = N / ROWS;
    const long per = (units + gridDim.x - 1) / gridDim.x;
    for (long u = order == 2 ? blockIdx.x * per : blockIdx.x; u < (order == 2 ? min(units, (blockIdx.x + 1) * per) : units); u += order == 2 ? 1 : gridDim.x) {
        long band;
        int g;
        if (order == 0) { band = u / ncg; g = (int)(u - band * ncg); }           // row band major: a band's column groups side by side
        else {                                                                    // (image, column group) major: bands of one group in a row
            const long pair = u / bands_img, bi = u - pair * bands_img;
            const long img = pair / ncg;
            g = (int)(pair - img * ncg);
            band = img * bands_img + bi;
        }
        const int col = (g * 16 + wave) * 256 + 4 * lane;
        if (col + 3 >= N) continue;
        float* p = dst + band * ROWS * ld + col;
#pragma unroll 16
        for (int r = 0; r < ROWS; ++r) {
            if (NT) {
                __builtin_nontemporal_store(v, p); __builtin_nontemporal_store(v, p + 1);
                __builtin_nontemporal_store(v, p + 2); __builtin_nontemporal_store(v, p + 3);
            } else {
                *reinterpret_cast<float4*>(p) = make_float4(v, v, v, v);
            }
            p += ld;
        }
    }
}
}  // namespace
extern "C" int gnms_profile_fill_tiles(float* dst, int B, int N, int64_t ld, int rows, int nontemporal, void* stream) {
    GNMS_CHECK_ARG(dst && B > 0 && N > 0 && ld >= N && ld % 4 == 0 && (uintptr_t)dst % 16 == 0,
                   "gnms_profile_fill_tiles: dst 16-byte aligned, ld >= N a multiple of 4");
    GNMS_CHECK_ARG((rows == 4 || rows == 8 || rows == 16 || rows == 32 || rows == 64) && N % rows == 0,
                   "gnms_profile_fill_tiles: rows per wave tile must be 4, 8, 16, 32 or 64 and divide N (rows=%d N=%d)", rows, N);
    const int order = 0;                                           // row band major (the other orders of round 2 measured slower: LABNOTES.md)
    const dim3 grid((unsigned)gnms_device_cu_count());
    hipStream_t st = (hipStream_t)stream;
    const long bands = (long)B * N / rows;
#define GNMS_FILL_TILES(R)                                                                                                                  \
    do {                                                                                                                                    \
        if (nontemporal) gnms_launch_prof(kProfPlainStream, prof_fill_tiles_kernel<R, true>, grid, dim3(1024), 0, st, dst, N, (long)ld, bands, 0.5f, order);   \
        else gnms_launch_prof(kProfPlainStream, prof_fill_tiles_kernel<R, false>, grid, dim3(1024), 0, st, dst, N, (long)ld, bands, 0.5f, order);            \
    } while (0)
    switch (rows) {
        case 4: GNMS_FILL_TILES(4); break;
        case 8: GNMS_FILL_TILES(8); break;
        case 16: GNMS_FILL_TILES(16); break;
        case 32: GNMS_FILL_TILES(32); break;
        default: GNMS_FILL_TILES(64); break;
    }
#undef GNMS_FILL_TILES
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
namespace {
// The store pattern of a SYMMETRIC matrix writer, with no arithmetic: upper-triangular T x T macro tiles, each written once where it
// is and once mirrored (rows <-> columns), row runs of T floats.  CPL floats per lane and store instruction: T / CPL lanes cover a row
// run, 64 / (T / CPL) row runs per instruction.  persist: one workgroup per CU walks a contiguous range of tiles (row-major over the
// upper triangle: a strip I, J = I .. end), else one workgroup per tile.
template <int T, int CPL, bool NT>
__global__ __launch_bounds__(1024) void prof_fill_sym_kernel(float* __restrict__ dst, int N, long ld, int nimg, int persist, float v) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    constexpr int LPR = T / CPL, RPI = 64 / LPR;
    const int RW = T / waves;
    const int nt = N / T;
    const long per_img = (long)nt * (nt + 1) / 2, total = per_img * nimg;
    long t0 = blockIdx.x, t1 = blockIdx.x + 1;
    if (persist) { t0 = total * blockIdx.x / gridDim.x; t1 = total * (blockIdx.x + 1) / gridDim.x; }
    const long step = persist == 2 ? gridDim.x : 1;                  // persist 2: round robin (one compact write frontier), else contiguous strips
    if (persist == 2) { t0 = blockIdx.x; t1 = total; }
    for (long t = t0; t < t1 && t < total; t += step) {
        const int img = (int)(t / per_img);
        long r = t - (long)img * per_img;
        int I = 0;
        while (r >= nt - I) { r -= nt - I; ++I; }                      // (a benchmark: the linear walk is a few dozen trips)
        const int J = I + (int)r;
        float* base = dst + (size_t)img * N * ld;
        auto put = [&](int R0, int C0) {
            for (int rr = 0; rr < RW; rr += RPI) {
                float* p = base + (size_t)(R0 + wave * RW + rr + lane / LPR) * ld + C0 + (lane % LPR) * CPL;
                if (NT) {
#pragma unroll
                    for (int j = 0; j < CPL; ++j) __builtin_nontemporal_store(v, p + j);
                } else if (CPL == 4) {
                    *reinterpret_cast<float4*>(p) = make_float4(v, v, v, v);
                } else {
                    *reinterpret_cast<float2*>(p) = make_float2(v, v);
                }
            }
        };
        put(I * T, J * T);
        if (I != J) put(J * T, I * T);
    }
}
}  // namespace
extern "C" int gnms_profile_fill_sym(float* dst, int B, int N, int64_t ld, int tile, int cols_per_lane, int nontemporal, int persist, void* stream) {
    GNMS_CHECK_ARG(dst && B > 0 && N > 0 && ld >= N && ld % 4 == 0 && (uintptr_t)dst % 16 == 0, "gnms_profile_fill_sym: dst 16-byte aligned, ld >= N a multiple of 4");
    GNMS_CHECK_ARG((tile == 128 || tile == 256) && N % tile == 0 && (cols_per_lane == 2 || cols_per_lane == 4) && tile / cols_per_lane <= 64,
                   "gnms_profile_fill_sym: tile 128 or 256 dividing N, 2 or 4 columns per lane");
    hipStream_t st = (hipStream_t)stream;
    const int nt = N / tile;
    const long total = (long)nt * (nt + 1) / 2 * B;
    const dim3 grid((unsigned)(persist ? gnms_device_cu_count() * (tile == 128 ? 2 : 1) : total));
    const dim3 block(tile == 128 ? 512 : 1024);
#define GNMS_FILL_SYM(TT, CC)                                                                                                              \
    do {                                                                                                                                   \
        if (nontemporal) gnms_launch_prof(kProfPlainStream, prof_fill_sym_kernel<TT, CC, true>, grid, block, 0, st, dst, N, (long)ld, B, persist, 0.5f);   \
        else gnms_launch_prof(kProfPlainStream, prof_fill_sym_kernel<TT, CC, false>, grid, block, 0, st, dst, N, (long)ld, B, persist, 0.5f);            \
    } while (0)
    if (tile == 128 && cols_per_lane == 2) GNMS_FILL_SYM(128, 2);
    else if (tile == 128) GNMS_FILL_SYM(128, 4);
    else GNMS_FILL_SYM(256, 4);
#undef GNMS_FILL_SYM
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
extern "C" int gnms_profile_fill(float* dst, size_t count, void* stream) {
    GNMS_CHECK_ARG(dst && count % 4 == 0 && (uintptr_t)dst % 16 == 0, "gnms_profile_fill: dst must be 16-byte aligned, count a multiple of 4");
    if (count == 0) return GNMS_OK;
    gnms_launch_prof(kProfPlainStream, prof_fill_kernel, dim3(256 * 16), dim3(512), 0, (hipStream_t)stream, reinterpret_cast<float4*>(dst), count / 4, 0.5f);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
extern "C" int gnms_profile_read(const float* src, size_t count, float* sink, void* stream) {
    GNMS_CHECK_ARG(src && sink && count % 4 == 0 && (uintptr_t)src % 16 == 0, "gnms_profile_read: src must be 16-byte aligned, count a multiple of 4");
    if (count == 0) return GNMS_OK;
    gnms_launch_prof(kProfPlainStream, prof_read_kernel, dim3(256 * 16), dim3(512), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(src), count / 4, sink);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

using namespace gnms;

// Profiling hook: re-runs ONLY the threshold bit-matrix kernel (K2, the one full read of the matrix) on a
// workspace that a previous gnms_forward filled (it needs `order`).  bench.py times it for the roofline line.
extern "C" int gnms_profile_bitmask(const float* iou, int B, int N, int64_t ld, const int32_t* counts, float nms_threshold,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    gnms_params P;
    gnms_default_params(&P);
    int rc = check_common("gnms_profile_bitmask", B, N, ld, &P, workspace, workspace_bytes);
    if (rc) return rc;
    if (B == 0 || N == 0) return GNMS_OK;
    P.nms_threshold = nms_threshold;
    return gnms_internal_launch_bitmask(make_call(B, N, counts, P, workspace, stream), iou, ld);
}

extern "C" int gnms_profile_bitmask_boxes(const float* boxes, int B, int N, const int32_t* counts, float nms_threshold, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    gnms_params P;
    gnms_default_params(&P);
    int rc = check_common("gnms_profile_bitmask_boxes", B, N, N, &P, workspace, workspace_bytes);
    if (rc) return rc;
    if (B == 0 || N == 0) return GNMS_OK;
    P.nms_threshold = nms_threshold;
    return gnms_internal_launch_bitmask_boxes(make_call(B, N, counts, P, workspace, stream), boxes);
}

// Profiling / test hook: ONLY the sorts (K1) of the 2D layer, on a chosen route, and what they leave in the workspace copied out.
namespace {
__global__ void export_sorts_kernel(int N, const int* __restrict__ counts, char* ws, gnms_ws_layout L, int has_boxes, int* __restrict__ order,
                                    int* __restrict__ rankof, float* __restrict__ sscore, float4* __restrict__ rbox, int* __restrict__ xidx,
                                    float4* __restrict__ xbox, int* __restrict__ flags) {
    using namespace gnms;
    const int b = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = gnms_count(counts, b, N);
    ImgPtrs I = img_ptrs(ws, L, b);
    if (k == 0 && flags) { flags[2 * b] = I.misc[2]; flags[2 * b + 1] = has_boxes ? I.misc[6] : 0; }
    if (k >= N) return;
    const size_t o = (size_t)b * N + k;
    if (order) order[o] = I.order[k];
    if (rankof) rankof[o] = I.rankof[k];
    if (sscore) sscore[o] = I.sscore[k];
    // (the sorts write these for the image's n boxes only: zeros behind them)
    const bool live = has_boxes && k < n;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (rbox) rbox[o] = live ? I.rbox[k] : zero;
    if (xidx) xidx[o] = live ? I.xidx[k] : 0;
    if (xbox) xbox[o] = live ? I.xbox[k] : zero;
}
}  // namespace

extern "C" int gnms_profile_sorts(const float* scores, const float* boxes, int B, int N, const int32_t* counts, int route, int32_t* order,
                                  int32_t* rankof, float* sscore, float* rbox, int32_t* xidx, float* xbox, int32_t* flags, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    gnms_params P;
    gnms_default_params(&P);
    int rc = check_common("gnms_profile_sorts", B, N, N, &P, workspace, workspace_bytes);
    if (rc) return rc;
    GNMS_CHECK_ARG(route >= 0 && route <= 3, "gnms_profile_sorts: route %d (0 default, 1 runs + merge, 2 ranked runs, 3 by histogram)", route);
    if (B == 0 || N == 0) return GNMS_OK;
    GNMS_CHECK_ARG(scores != nullptr, "gnms_profile_sorts: scores is NULL");
    const LayerCall c = make_call(B, N, counts, P, workspace, stream);
    if ((rc = gnms_internal_launch_sorts(c, scores, boxes, 0, route))) return rc;
    if (order || rankof || sscore || rbox || xidx || xbox || flags) {
        export_sorts_kernel<<<dim3(gnms_div_up(N, 256), B), 256, 0, c.st>>>(N, counts, c.ws, c.L, boxes ? 1 : 0, order, rankof, sscore,
                                                                          (float4*)rbox, xidx, (float4*)xbox, flags);
        GNMS_CHECK_LAUNCH();
    }
    return GNMS_OK;
}

namespace {
__global__ void export_sort_paths_kernel(char* ws, gnms_ws_layout L, int B, int32_t* __restrict__ paths) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * B) paths[i] = gnms::img_ptrs(ws, L, i >> 1).misc[gnms::kSortPathSlot + (i & 1)];
}
}  // namespace

extern "C" int gnms_profile_sort_paths(int B, int N, int32_t* paths, int32_t* cap_out, void* workspace, size_t workspace_bytes, void* stream) {
    gnms_params P;
    gnms_default_params(&P);
    int rc = check_common("gnms_profile_sort_paths", B, N, N, &P, workspace, workspace_bytes);
    if (rc) return rc;
    if (cap_out) *cap_out = gnms_internal_hist_cap().load();
    if (B == 0 || N == 0 || !paths) return GNMS_OK;
    const LayerCall c = make_call(B, N, nullptr, P, workspace, stream);
    export_sort_paths_kernel<<<gnms_div_up(2 * B, 64), 64, 0, c.st>>>(c.ws, c.L, B, paths);
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}

extern "C" int gnms_profile_set_hist_cap(int cap) {
    return gnms_internal_hist_cap().exchange(cap < 0 ? gnms::kHistCap : std::min(cap, gnms::kHistCapMax));
}
