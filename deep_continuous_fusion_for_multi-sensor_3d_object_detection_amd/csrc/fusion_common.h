// fusion_common.h -- device helpers shared by fusion.hip and fusion_det.hip: the bilinear taps of the point sampler, the
// BEV pixel centre, the per-frame strides of the batched launches.
#pragma once
#include "dcf_common.h"

namespace {

struct Taps {
    int x0, x1, y0, y1;
    float w00, w01, w10, w11;
};

// ix = u/4 - 0.5, iy = v/4 - 0.5 on the stride-4 map, border clamp (oracle/model_ref.py bilinear_sample)
__device__ __forceinline__ Taps make_taps(float u, float v, int Hf, int Wf)
{
    const float ix = u * 0.25f - 0.5f, iy = v * 0.25f - 0.5f;
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float wx = ix - x0f, wy = iy - y0f;
    Taps t;
    const int x0 = (int)x0f, y0 = (int)y0f;
    t.x0 = min(max(x0, 0), Wf - 1); t.x1 = min(max(x0 + 1, 0), Wf - 1);
    t.y0 = min(max(y0, 0), Hf - 1); t.y1 = min(max(y0 + 1, 0), Hf - 1);
    t.w00 = (1.f - wy) * (1.f - wx); t.w01 = (1.f - wy) * wx;
    t.w10 = wy * (1.f - wx); t.w11 = wy * wx;
    return t;
}

// Batched launches (grid.y = frame of the batch): element strides between the frames' tensors; all zero for a single frame.
struct FrameStride {
    int64_t a, b, c, d, e;
};

struct FuseGeom {
    int h, w, stride, K;
    float xs, xo, ys, yo;
};

__device__ __forceinline__ void pixel_centre(const FuseGeom &g, int i, int j, float &X, float &Y)
{
    const float s = (float)g.stride;
    X = __fdiv_rn(__fsub_rn(__fmul_rn((float)i + 0.5f, s), g.xo), g.xs);
    Y = __fdiv_rn(__fsub_rn(__fmul_rn((float)j + 0.5f, s), g.yo), g.ys);
}

}  // namespace
