// bbox_decode.h -- the 2D box decode of lib/rpn_util.py:886-934 for ONE anchor, shared by gnms_bbox_transform_inv (proposals.hip,
// every anchor) and gnms_detect3d_decode (detect3d.hip, the selected anchors only): one definition, so the two routes cannot drift
// apart by a bit.
#pragma once
#include <hip/hip_runtime.h>

// b = anchor (x1 y1 x2 y2), d = deltas (dx dy dw dh) -> predicted (x1 y1 x2 y2); the reference's operation order
__device__ __forceinline__ float4 gnms_bbox_decode(const float4 b, float4 d, const float4 means, const float4 stds, const int use_means,
                                                   const int use_stds) {
    const float widths = b.z - b.x + 1.0f;                              // :887
    const float heights = b.w - b.y + 1.0f;                             // :888
    const float ctr_x = b.x + 0.5f * widths;                            // :889
    const float ctr_y = b.y + 0.5f * heights;                           // :890
    if (use_stds) { d.x *= stds.x; d.y *= stds.y; d.z *= stds.z; d.w *= stds.w; }       // :903-907
    if (use_means) { d.x += means.x; d.y += means.y; d.z += means.z; d.w += means.w; }   // :909-913
    const float pcx = d.x * widths + ctr_x;                             // :915
    const float pcy = d.y * heights + ctr_y;                            // :916
    const float pw = expf(d.z) * widths;                                // :917
    const float ph = expf(d.w) * heights;                               // :918
    return make_float4(pcx - 0.5f * pw, pcy - 0.5f * ph, pcx + 0.5f * pw - 1.0f, pcy + 0.5f * ph - 1.0f);   // :924-934
}
