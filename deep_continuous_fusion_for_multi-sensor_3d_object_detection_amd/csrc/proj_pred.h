// proj_pred.h -- the projection's keep predicate and its fp32 chain, shared by the projection / compaction kernels
// (geometry.hip) and the camera visibility mask (camera_mask.hip): one spelling, so the mask decides what the projection decides.
//
// Bit-exactness contract (checked against oracle/dcf_oracle.c and visibility.project_chain): every file that includes this is
// compiled with -ffp-contract=off, and every fused step is spelled __fmaf_rn, so each product/sum rounds exactly where the
// reference's CPU arithmetic rounds.
#pragma once
#include "dcf_common.h"

namespace {

struct Lim6 { float v[6]; };
struct Crt12 { float v[12]; };

__device__ __forceinline__ bool in_range(float x, float y, float z, const Lim6 &l)
{
    return x > l.v[0] && x < l.v[1] && y > l.v[2] && y < l.v[3] && z > l.v[4] && z < l.v[5];
}

// data_import_carla.py:196-205 on top of the range filter of :215-226
struct ProjPred {
    Lim6 lim;
    Crt12 c;
    float ulim, vlim;
    int mode;
    __device__ bool operator()(const float *pts, int i, float *u, float *v) const
    {
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        if (!in_range(x, y, z, lim)) return false;
        float a[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float t = __fmul_rn(x, c.v[j]);       // the reference's K=4 sgemm chain
            t = __fmaf_rn(y, c.v[3 + j], t);
            t = __fmaf_rn(z, c.v[6 + j], t);
            t = __fmaf_rn(1.0f, c.v[9 + j], t);
            a[j] = t;
        }
        const float uu = __fdiv_rn(a[0], a[2]), vv = __fdiv_rn(a[1], a[2]);
        *u = uu;
        *v = vv;
        bool keep = uu > 0.0f && uu < ulim && vv > 0.0f && vv < vlim;
        if (mode == DCF_PROJ_CORRECT) keep = keep && a[2] > 0.0f;
        return keep;
    }
};

// ProjPred's chain for a caller that needs the depth a2 as well, and needs it for rows outside the range too (the camera mask's
// occlusion test): the statements of the loop above, so the compiler folds the two where a kernel uses both.
__device__ __forceinline__ void proj_chain(float x, float y, float z, const Crt12 &c, float &u, float &v, float &a2)
{
    float a[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float t = __fmul_rn(x, c.v[j]);
        t = __fmaf_rn(y, c.v[3 + j], t);
        t = __fmaf_rn(z, c.v[6 + j], t);
        t = __fmaf_rn(1.0f, c.v[9 + j], t);
        a[j] = t;
    }
    u = __fdiv_rn(a[0], a[2]);
    v = __fdiv_rn(a[1], a[2]);
    a2 = a[2];
}

}  // namespace
