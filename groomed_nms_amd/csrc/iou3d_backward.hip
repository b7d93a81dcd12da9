// iou3d_backward.hip -- gnms_iou3d_backward: the cotangent of a pairwise 3D overlap matrix (gnms_iou3d_from_params, method 0 / 1 / 2,
// gnms_nms_overlap3d_from_params) contracted with d overlap / d cuboid.
// pair_grad_walker.h's walker and reduce with the 3D geometry: iou3d_records_kernel first builds the boxes' records (the forward's
// floats: corners_of + aabb_record; the backward keeps the first eight floats of a record), which is what the walker reads.  Six extent
// sums per box, two 64-column sub-tiles per unit (12 column accumulators a lane against the 2D geometry's 16), the pair arithmetic of
// iou3d_grad.h<METHOD>, a slab element three float2; the reduce carries the six extent sums of a box to its seven parameters (stage 1,
// once per box).
#include "iou3d_grad.h"
#include "pair_grad_walker.h"

namespace {

using namespace gnms_iou3d_grad;

constexpr int kRec8 = 8;                         // floats kept per box: u | v of the record

__global__ __launch_bounds__(256) void iou3d_records_kernel(const float* __restrict__ params, long count, float* __restrict__ rec) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float4 u, v, e;
    record_of_params(params + i * 7, u, v, e);
    float4* o = reinterpret_cast<float4*>(rec + i * kRec8);
    o[0] = u; o[1] = v;
}

// The FORMS below are load-bearing for the walker's register allocation, not taste (LABNOTES R17.2): the state is Rec plus the record's
// unread eighth float (not the two float4 as loaded); load / stash / unstash / bcast take and return it BY VALUE, pair / add_grad BY
// REFERENCE; stash / unstash get the column's address.  Each of them, changed, moves the nine walkers off the instruction streams they
// have had since they were a copy of the 2D kernel.  Compare streams and tools/kernel_resources.sh rows after touching any.
struct Iou3dCuboids {                            // everything but the pair arithmetic: the reduce is compiled once, not per METHOD
    static constexpr int kAcc = 6, kSubTiles = 2, kWalkFloats = kRec8, kStash4 = 2, kBoxFloats = 7;
    static constexpr bool kAlign16 = false;
    static constexpr const char* kWhat = "params";
    struct Box {
        Rec r;
        float w;                                                      // the record's eighth float: stashed with the rest, never read
    };
    using Pair = gnms_iou3d_grad::Pair;
    static __device__ __forceinline__ Box of(const float4 u, const float4 v) { return Box{rec_of(u, v), v.w}; }
    static __device__ __forceinline__ Box load(const float* __restrict__ recs, size_t i) {
        const float4* r = reinterpret_cast<const float4*>(recs) + i * 2;
        return of(r[0], r[1]);
    }
    static __device__ __forceinline__ void stash(float4* at, const Box b) {
        at[0] = make_float4(b.r.vol, b.r.y0, b.r.y1, b.r.x0);
        at[1] = make_float4(b.r.x1, b.r.z0, b.r.z1, b.w);
    }
    static __device__ __forceinline__ Box unstash(const float4* at) { return Box{rec_of(at[0], at[1]), 0.0f}; }
    static __device__ __forceinline__ Box bcast(const Box b, int lane) {
        using gnms_pair_grad::bcast;
        Box o;
        o.r.x0 = bcast(b.r.x0, lane); o.r.x1 = bcast(b.r.x1, lane); o.r.y0 = bcast(b.r.y0, lane); o.r.y1 = bcast(b.r.y1, lane);
        o.r.z0 = bcast(b.r.z0, lane); o.r.z1 = bcast(b.r.z1, lane); o.r.vol = bcast(b.r.vol, lane);
        o.w = 0.0f;
        return o;
    }
    static __device__ __forceinline__ Pair pair(const Box& a, const Box& b) { return pair_of(a.r, b.r); }
    static __device__ __forceinline__ void store_slab(float* __restrict__ slab, size_t i, const float (&acc)[6]) {
        float2* o = reinterpret_cast<float2*>(slab + i * 6);
        o[0] = make_float2(acc[0], acc[1]); o[1] = make_float2(acc[2], acc[3]); o[2] = make_float2(acc[4], acc[5]);
    }
    static __device__ __forceinline__ void add_slab(float (&s)[6], const float* __restrict__ slab, size_t i) {
        const float* v = slab + i * 6;
        const float2 a = reinterpret_cast<const float2*>(v)[0], b = reinterpret_cast<const float2*>(v)[1], c = reinterpret_cast<const float2*>(v)[2];
        s[0] += a.x; s[1] += a.y; s[2] += b.x; s[3] += b.y; s[4] += c.x; s[5] += c.y;
    }
    static __device__ __forceinline__ void finish(const float* params, float* d, size_t i, const float (&s)[6]) {
        const size_t o = i * 7;
        float g[7];
        params_grad(params + o, s, g);
#pragma unroll
        for (int k = 0; k < 7; ++k) d[o + k] = g[k];
    }
    static size_t records_bytes(long boxes) { return gnms_align_up((size_t)boxes * kRec8 * sizeof(float), 256); }
    static int prepare(const float* params, long boxes, float* rec, hipStream_t st) {
        iou3d_records_kernel<<<(unsigned)((boxes + 255) / 256), 256, 0, st>>>(params, boxes, rec);
        GNMS_CHECK_LAUNCH();
        return GNMS_OK;
    }
};

template <int METHOD>
struct Iou3dGeometry : Iou3dCuboids {
    using Sums = Iou3dCuboids;
    static __device__ __forceinline__ void add_grad(const Box& s, const Box& o, const Pair& p, float g, float (&acc)[6]) {
        add_extent_grad<METHOD>(s.r, o.r, p, g, acc);
    }
};

}  // namespace

extern "C" size_t gnms_iou3d_backward_workspace_bytes(int B, int M, int N) {
    if (B <= 0 || M <= 0 || N <= 0) return 0;
    return gnms_pair_grad::workspace_bytes<Iou3dGeometry<0>>(B, M, N, false);   // (the one-set form needs no second record array: it fits as well)
}

extern "C" int gnms_iou3d_backward(const float* params_a, const float* params_b, const float* grad, int B, int M, int N, int64_t ld, int method,
                                   float* d_params_a, float* d_params_b, void* workspace, size_t workspace_bytes, void* stream) {
    GNMS_CHECK_ARG(B >= 0 && M >= 0 && N >= 0, "gnms_iou3d_backward: negative size (B=%d M=%d N=%d)", B, M, N);   // (in front of the method, as ever)
    GNMS_CHECK_ARG(method >= 0 && method <= 2, "gnms_iou3d_backward: method %d not in {0,1,2}", method);
#define GNMS_IOU3D_BWD(METHOD)                                                                                                                 \
    gnms_pair_grad::backward<Iou3dGeometry<METHOD>>("gnms_iou3d_backward", params_a, params_b, grad, B, M, N, ld, d_params_a, d_params_b, workspace, \
                                                    workspace_bytes, stream)
    return method == 0 ? GNMS_IOU3D_BWD(0) : method == 1 ? GNMS_IOU3D_BWD(1) : GNMS_IOU3D_BWD(2);
#undef GNMS_IOU3D_BWD
}
