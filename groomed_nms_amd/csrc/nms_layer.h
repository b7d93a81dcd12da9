// nms_layer.h -- what the translation units of the NMS layer share: nms_layer.hip (the entries and every launcher but the two below), the
// nms_tail_*.hip and nms_tail_write_*.hip units (launch_tail / launch_tail_write with their kernels, one overlap source per unit) and
// nms_profile.hip (the measurement entries).  Host code only: no kernel and no __device__ function.
//
// Everything declared here has ONE definition, in nms_layer.hip where nothing else is said.  Process-wide state (the switches' function-local
// statics, the caches behind allow_lds and gnms_device_cu_count, the histogram cap) therefore exists once and is reached through these
// functions: a switch is read once per process, whichever unit asks.
#pragma once
#include <atomic>
#include "gnms_common.h"

namespace gnms {

int next_pow2(int n);

// block_sort<E>: P = threads * E.  P <= 1024 -> E = 1; above, 1024 threads and E = P / 1024 (N <= 16384 -> E <= 16).
#define GNMS_DISPATCH_SORT(P2, ...)                               \
    do {                                                          \
        const int e__ = (P2) <= 1024 ? 1 : (P2) / 1024;           \
        if (e__ == 1) { constexpr int E = 1; __VA_ARGS__; }              \
        else if (e__ == 2) { constexpr int E = 2; __VA_ARGS__; }         \
        else if (e__ == 4) { constexpr int E = 4; __VA_ARGS__; }         \
        else if (e__ == 8) { constexpr int E = 8; __VA_ARGS__; }         \
        else { constexpr int E = 16; __VA_ARGS__; }                      \
    } while (0)

size_t leaders_lds_bytes(int N);

template <typename K>
int allow_lds(K kernel, size_t bytes) { return gnms_allow_lds_raw(reinterpret_cast<const void*>(kernel), bytes); }

int check_common(const char* fn, int B, int N, int64_t ld, const gnms_params* P, const void* ws, size_t ws_bytes);

// the developer / test switches (each reads its environment variable once; see the definitions)
int env_switch(const char* name, int dflt);
int w_write_through_routes();          // GNMS_W_WRITE_THROUGH
bool matrix_sym_detection(int N);      // GNMS_MATRIX_SYM
bool fast_tail_enabled();              // GNMS_FAST_TAIL
bool one_launch_enabled();             // GNMS_ONE_LAUNCH

// dynamic LDS of the chain in tail_kernel / tail_write_kernel; P2: the launch's key count (>= 1024: the fused kernels always run 1024 threads)
size_t tail_lds_bytes(int N, int P2, int fast);
// 3D: the write role of the tail launch as symmetric writers (writers_sym_persistent)
bool sym_writers_in_tail_launch(int N, int64_t ld, const float* out);

// What every launcher of the layer is handed: the sizes, the workspace, the stream and the outputs of one call.
struct LayerCall {
    int B, N;
    const int32_t* counts;
    gnms_params P;
    gnms_ws_layout L;
    char* ws;
    hipStream_t st;
    int P2;                                                       // keys of the block sorts: next_pow2(N)
    float* prob;
    int64_t *order, *valid, *invalid;
    int32_t *nvalid, *ninvalid;
    size_t sort_lds() const { return (size_t)P2 * 8; }
    int sort_threads() const { return P2 <= 1024 ? P2 : 1024; }
};
LayerCall make_call(int B, int N, const int32_t* counts, const gnms_params& P, void* workspace, void* stream, float* prob = nullptr,
                    int64_t* order = nullptr, int64_t* valid = nullptr, int64_t* invalid = nullptr, int32_t* nvalid = nullptr,
                    int32_t* ninvalid = nullptr);
// The prologue of an entry: the checks, then the call.  kCallEmpty (> 0: not an error code): nothing to launch -- B == 0, or N == 0, where the
// counts the call has are zeroed.  without_matrix: an entry that has the boxes only, the grouped hard-sorted modes; ptrs_ok: the entry's own
// pointers are all there (asked only of a call that is not empty; null_msg says which entry).
constexpr int kCallEmpty = 1;
int begin_call(const char* fn, LayerCall* c, int B, int N, int64_t ld, const int32_t* counts, const gnms_params* params, void* workspace,
               size_t workspace_bytes, void* stream, bool without_matrix, bool ptrs_ok, const char* null_msg, float* prob = nullptr,
               int64_t* order = nullptr, int64_t* valid = nullptr, int64_t* invalid = nullptr, int32_t* nvalid = nullptr, int32_t* ninvalid = nullptr);
// the entries return through this: an empty call is a success
#define GNMS_BEGIN_CALL(...)                                      \
    do {                                                          \
        const int rc__ = begin_call(__VA_ARGS__);                 \
        if (rc__) return rc__ == kCallEmpty ? GNMS_OK : rc__;     \
    } while (0)

}  // namespace gnms

// ------------------------------------------------------------------------------------------------
// the launchers that cross a unit (their descriptions stand at the definitions)
// ------------------------------------------------------------------------------------------------
// nms_layer.hip; called by nms_profile.hip as well
int gnms_internal_launch_sorts(const gnms::LayerCall& c, const float* scores, const float* boxes, int mode3d = 0, int route = 0);
int gnms_internal_launch_bitmask(const gnms::LayerCall& c, const float* iou, int64_t ld, int full = 0);
int gnms_internal_launch_bitmask_boxes(const gnms::LayerCall& c, const float* boxes);
// keys in one bin from which on sort_hist_rank_kernel falls back to the run sort (gnms_profile_set_hist_cap moves it)
std::atomic<int>& gnms_internal_hist_cap();

// K3..K6 in one launch (tail_kernel) and K3..K6 + the matrix write in one launch (tail_write_kernel).  Only DECLARED here: the definitions are
// in nms_tail_launch.h / nms_tail_write_launch.h, which the nms_tail_<source>.hip / nms_tail_write_<source>.hip units alone include, one
// explicit instantiation each.  A unit that calls a launcher cannot instantiate its kernels a second time (they sit in anonymous namespaces,
// so a second copy would build without complaint): a source without a unit of its own is a link error.
template <int SRC>
int gnms_internal_launch_tail(const gnms::LayerCall& c, const float* src, int64_t ld, int sym, int chain_cap = 0);
extern template int gnms_internal_launch_tail<gnms::kFromMatrix>(const gnms::LayerCall&, const float*, int64_t, int, int);
extern template int gnms_internal_launch_tail<gnms::kFromBoxes>(const gnms::LayerCall&, const float*, int64_t, int, int);
extern template int gnms_internal_launch_tail<gnms::kFromRecords>(const gnms::LayerCall&, const float*, int64_t, int, int);
template <int SRC>
int gnms_internal_launch_tail_write(const gnms::LayerCall& c, const float* chain_src, const float* write_src, float* out, int64_t ld);
extern template int gnms_internal_launch_tail_write<gnms::kFromBoxes>(const gnms::LayerCall&, const float*, const float*, float*, int64_t);
extern template int gnms_internal_launch_tail_write<gnms::kFromRecords>(const gnms::LayerCall&, const float*, const float*, float*, int64_t);
