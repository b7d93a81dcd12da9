// optim.hip -- the optimiser step of the reference's loop (lib/core.py:99-113: clip_grad_value_, torch.optim.SGD.step, zero_grad; DESIGN.md
// 3.22) for a whole parameter group in one launch.
//
//   gnms_sgd_step   per element, float32, every operation rounded on its own (-ffp-contract=off, build.py):
//                       g' = g < -c ? -c : (g > c ? c : g)      NaN stays NaN (torch.clamp)
//                       d  = g' + wd * p
//                       buf = mo * buf + d
//                       p  = p + (-lr) * buf
//                       g  = 0
//
// Table driven: a tensor table (p, g, buf, numel) and a task table (tensor, start, count, kind), both int64 [..][4] on the device; a task is
// at most one chunk of one tensor, and the workgroups loop over the tasks, so a BatchNorm vector of 64 elements costs one pass of one
// workgroup's loop, not a workgroup.  A task of kind 1 has p, g and buf on 16 bytes at its start and moves 16 bytes per lane and stream
// (its last count % 4 elements one by one); a task of kind 0 (a tensor's head up to the first 16-byte boundary, or a tensor whose three
// arrays do not share their misalignment) moves 4.  Each element is read once and written once: six streams, 24 bytes per parameter.
//
// The gate and the schedule are read on the device: the loss (a float32 scalar; the update is applied only where loss > 0, lib/core.py:102,
// so not for NaN) and, in the capturable form, the iteration counter state[0] that indexes the float64 schedule.  The launch advances
// the counter itself.  Every workgroup reads state[0] before it takes a ticket on state[1]; the holder of the last ticket, after which
// no workgroup has its read still ahead of it, writes state[0] + 1 and resets the ticket.  No float atomics, no workspace.
#include <limits.h>

#include "gnms_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWorkgroupsPerCu = 4;                     // 16 waves per CU, each with three 16-byte loads per lane in flight

typedef float f4 __attribute__((ext_vector_type(4)));
// the addresses come out of a table of integers: say that they are global memory, or every access is a flat one
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f4 gf4;

struct sgd_consts {
    float neg_lr, mo, wd, c;
    int use_clip;
};

template <bool kNT> __device__ __forceinline__ f4 load_once(const gf4* p) {
    return kNT ? __builtin_nontemporal_load(p) : *p;
}
template <bool kNT> __device__ __forceinline__ void store_once(gf4* p, f4 v) {
    if (kNT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

__device__ __forceinline__ void sgd_update(float g, float& p, float& b, const sgd_consts& k) {
    if (k.use_clip) g = g < -k.c ? -k.c : (g > k.c ? k.c : g);
    const float d = g + k.wd * p;
    b = k.mo * b + d;
    p = p + k.neg_lr * b;
}

// kNT: bit 0 = the three 16-byte loads non-temporal, bit 1 = the three 16-byte stores
template <int kNT>
__global__ __launch_bounds__(kThreads) void sgd_step_kernel(const long long* __restrict__ tensors, int n_tensors,
                                                            const long long* __restrict__ tasks, int n_tasks, sgd_consts k,
                                                            const float* __restrict__ loss, const double* __restrict__ lr_table,
                                                            int lr_len, long long* state, int advance) {
    __shared__ long long s_it;
    if (threadIdx.x == 0) s_it = __hip_atomic_load(&state[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();                                    // the read has returned: its value lies in LDS
    const long long it = s_it;
    if (lr_table) {
        const long long e = it < 0 ? 0 : (it >= lr_len ? lr_len - 1 : it);
        k.neg_lr = (float)(-lr_table[e]);
    }
    const bool apply = loss ? (*loss > 0.0f) : true;    // false for NaN

    for (int t = blockIdx.x; t < n_tasks; t += gridDim.x) {
        const long long* __restrict__ tk = tasks + (size_t)t * GNMS_SGD_ROW;
        const long long ti = tk[0], start = tk[1], count = tk[2], kind = tk[3];
        if (ti < 0 || ti >= n_tensors) continue;        // uniform: a task that does not lie inside its tensor touches nothing
        const long long* __restrict__ tn = tensors + (size_t)ti * GNMS_SGD_ROW;
        const long long numel = tn[3];
        if (start < 0 || count < 0 || numel < 0 || start > numel || count > numel - start) continue;
        gfloat* __restrict__ p = (gfloat*)(uintptr_t)tn[0] + start;
        gfloat* __restrict__ g = (gfloat*)(uintptr_t)tn[1] + start;
        gfloat* __restrict__ b = (gfloat*)(uintptr_t)tn[2] + start;
        long long done = 0;
        if (kind == 1 && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)b) & 15) == 0) {
            const long long nvec = count >> 2;
            gf4* __restrict__ p4 = (gf4*)p;
            gf4* __restrict__ g4 = (gf4*)g;
            gf4* __restrict__ b4 = (gf4*)b;
            const f4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
            for (long long i = threadIdx.x; i < nvec; i += kThreads) {
                if (apply) {
                    const f4 gv = load_once<(kNT & 1) != 0>(g4 + i);
                    const f4 pv = load_once<(kNT & 1) != 0>(p4 + i);
                    const f4 bv = load_once<(kNT & 1) != 0>(b4 + i);
                    float pe[4] = {pv.x, pv.y, pv.z, pv.w}, be[4] = {bv.x, bv.y, bv.z, bv.w};
                    const float ge[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) sgd_update(ge[e], pe[e], be[e], k);
                    const f4 bo = {be[0], be[1], be[2], be[3]}, po = {pe[0], pe[1], pe[2], pe[3]};
                    store_once<(kNT & 2) != 0>(b4 + i, bo);
                    store_once<(kNT & 2) != 0>(p4 + i, po);
                }
                store_once<(kNT & 2) != 0>(g4 + i, zero);
            }
            done = nvec << 2;
        }
        for (long long i = done + threadIdx.x; i < count; i += kThreads) {      // a vector task's tail, or a scalar task
            if (apply) {
                float pv = p[i], bv = b[i];
                sgd_update(g[i], pv, bv, k);
                b[i] = bv;
                p[i] = pv;
            }
            g[i] = 0.f;
        }
    }

    if (threadIdx.x == 0 && advance) {
        const unsigned long long ticket = atomicAdd(reinterpret_cast<unsigned long long*>(&state[1]), 1ull);
        if (ticket == (unsigned long long)gridDim.x - 1) {                      // every workgroup has read state[0]
            __hip_atomic_store(&state[1], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&state[0], it + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

extern "C" int gnms_sgd_step(const int64_t* tensors, int n_tensors, const int64_t* tasks, int n_tasks, double lr, double momentum,
                             double weight_decay, double clip_value, int use_clip, const float* loss, const double* lr_table,
                             int lr_table_len, int64_t* state, int advance, int grid, int nt, void* stream) {
    GNMS_CHECK_ARG(n_tensors >= 0 && n_tasks >= 0, "gnms_sgd_step: n_tensors=%d n_tasks=%d", n_tensors, n_tasks);
    GNMS_CHECK_ARG(state, "gnms_sgd_step: state (int64 [2] on the device: iteration, ticket) missing");
    GNMS_CHECK_ARG(n_tasks == 0 || (tensors && tasks && n_tensors > 0), "gnms_sgd_step: %d tasks without tables", n_tasks);
    GNMS_CHECK_ARG((((uintptr_t)tensors | (uintptr_t)tasks | (uintptr_t)state | (uintptr_t)lr_table) & 7) == 0 && ((uintptr_t)loss & 3) == 0,
                   "gnms_sgd_step: tables, state and lr_table must be 8-byte aligned, loss 4-byte aligned");
    GNMS_CHECK_ARG(!lr_table || lr_table_len >= 1, "gnms_sgd_step: lr_table of %d entries", lr_table_len);
    GNMS_CHECK_ARG(!use_clip || clip_value >= 0, "gnms_sgd_step: clip_value=%g (>= 0, or use_clip = 0)", clip_value);
    GNMS_CHECK_ARG(grid >= 0 && nt >= 0 && nt <= 3, "gnms_sgd_step: grid=%d nt=%d (grid >= 0; nt: bit 0 loads, bit 1 stores)", grid, nt);
    if (n_tasks == 0 && !advance) return GNMS_OK;
    sgd_consts k;
    k.neg_lr = (float)(-lr);
    k.mo = (float)momentum;
    k.wd = (float)weight_decay;
    k.c = use_clip ? (float)clip_value : 0.f;
    k.use_clip = use_clip ? 1 : 0;
    int blocks = grid > 0 ? grid : gnms_device_cu_count() * kWorkgroupsPerCu;
    if (blocks > n_tasks) blocks = n_tasks;
    if (blocks < 1) blocks = 1;                         // no tasks: one workgroup still advances the counter
#define GNMS_SGD_LAUNCH(NT)                                                                                                     \
    sgd_step_kernel<NT><<<blocks, kThreads, 0, (hipStream_t)stream>>>((const long long*)tensors, n_tensors, (const long long*)tasks, n_tasks, k, \
                                                                       loss, lr_table, lr_table_len, (long long*)state, advance)
    switch (nt) {
        case 0: GNMS_SGD_LAUNCH(0); break;
        case 1: GNMS_SGD_LAUNCH(1); break;
        case 2: GNMS_SGD_LAUNCH(2); break;
        default: GNMS_SGD_LAUNCH(3); break;
    }
#undef GNMS_SGD_LAUNCH
    GNMS_CHECK_LAUNCH();
    return GNMS_OK;
}
