// iou_backward.hip -- gnms_iou2d_backward: the cotangent of a pairwise 2D IoU matrix contracted with dIoU/dbox.
// pair_grad_walker.h's walker and reduce with the 2D geometry: four coordinate sums per box, four 64-column sub-tiles per unit
// (32 rows x 256 columns a chunk row), the pair arithmetic of iou_grad.h, a slab element and the result one float4.
#include "iou_grad.h"
#include "pair_grad_walker.h"

namespace {

struct Iou2dGeometry {
    static constexpr int kAcc = 4, kSubTiles = 4, kWalkFloats = 4, kStash4 = 1, kBoxFloats = 4;
    static constexpr bool kAlign16 = true;                           // a box is loaded, a gradient stored, as one float4
    static constexpr const char* kWhat = "boxes";
    struct Box {
        float4 b;
        float area;                                                   // carried in a register, broadcast with the box; not stashed
    };
    using Pair = gnms_iou_grad::Pair;
    using Sums = Iou2dGeometry;
    static __device__ __forceinline__ Box of(const float4 b) { return Box{b, gnms_iou_grad::box_area(b)}; }
    static __device__ __forceinline__ Box load(const float* __restrict__ boxes, size_t i) { return of(*reinterpret_cast<const float4*>(boxes + i * 4)); }
    static __device__ __forceinline__ void stash(float4* at, const Box v) { at[0] = v.b; }
    static __device__ __forceinline__ Box unstash(const float4* at) { return of(at[0]); }
    static __device__ __forceinline__ Box bcast(const Box v, int lane) {
        using gnms_pair_grad::bcast;
        Box o;
        o.b = make_float4(bcast(v.b.x, lane), bcast(v.b.y, lane), bcast(v.b.z, lane), bcast(v.b.w, lane));
        o.area = bcast(v.area, lane);
        return o;
    }
    static __device__ __forceinline__ Pair pair(const Box& a, const Box& b) { return gnms_iou_grad::pair_of(a.b, a.area, b.b, b.area); }
    static __device__ __forceinline__ void add_grad(const Box& s, const Box& o, const Pair& p, float g, float (&acc)[4]) {
        gnms_iou_grad::add_box_grad(s.b, o.b, p, g, acc);
    }
    static __device__ __forceinline__ void store_slab(float* __restrict__ slab, size_t i, const float (&acc)[4]) {
        *reinterpret_cast<float4*>(slab + i * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
    static __device__ __forceinline__ void add_slab(float (&s)[4], const float* __restrict__ slab, size_t i) {
        const float4 v = reinterpret_cast<const float4*>(slab)[i];
        s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
    }
    static __device__ __forceinline__ void finish(const float* __restrict__, float* __restrict__ d, size_t i, const float (&s)[4]) {
        reinterpret_cast<float4*>(d)[i] = make_float4(s[0], s[1], s[2], s[3]);
    }
    // the walker reads the boxes themselves
    static size_t records_bytes(long) { return 0; }
    static int prepare(const float*, long, float*, hipStream_t) { return GNMS_OK; }
};

}  // namespace

extern "C" size_t gnms_iou2d_backward_workspace_bytes(int B, int M, int N) {
    if (B <= 0 || M <= 0 || N <= 0) return 0;
    return gnms_pair_grad::workspace_bytes<Iou2dGeometry>(B, M, N, false);
}

extern "C" int gnms_iou2d_backward(const float* boxes_a, const float* boxes_b, const float* grad, int B, int M, int N, int64_t ld,
                                   float* d_boxes_a, float* d_boxes_b, void* workspace, size_t workspace_bytes, void* stream) {
    return gnms_pair_grad::backward<Iou2dGeometry>("gnms_iou2d_backward", boxes_a, boxes_b, grad, B, M, N, ld, d_boxes_a, d_boxes_b, workspace,
                                                   workspace_bytes, stream);
}
