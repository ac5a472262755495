// ev_geom.h -- the fp64 rotated-rectangle geometry shared by the evaluation post-processing (evalpost.hip) and the anchor
// assignment of `loss_sampling: anchor` (loss.hip): rectangle corners, Sutherland-Hodgman clip, shoelace area, bird's-eye IoU.
// evalgeom.py / evalrank.bev_iou are the host statements; tests/test_gpu_eval.py and tests/test_gpu_eval_ranked.py pin these functions
// through the evaluation kernels, and tests/test_gpu_iou_exact.py pins them to an exact rational clip where an edge of one rectangle
// lies on the line of an edge of the other up to rounding (tests/test_iou_exact_host.py does the same for the host statement, and shows
// that no pass holds more than 8 vertices there).  ev_clip keeps two 12-vertex polygons per lane in scratch.
#pragma once
#include "dcf_common.h"

namespace {

__device__ double ev_shoelace(const double (*p)[2], int n)
{
    double a = 0.0, b = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = (i + n - 1) % n;                  // roll(., 1)[i] = [i - 1]
        a += p[i][0] * p[j][1];
        b += p[i][1] * p[j][0];
    }
    return 0.5 * fabs(a - b);
}

// Intersection polygon of `subject` (4 vertices) with the convex polygon `clip` (4 vertices), half-plane by half-plane;
// strictly-left-of-edge is inside (evalgeom._clip_convex).  Returns the vertex count (<= 8).
__device__ int ev_clip(const double (*subject)[2], const double (*clip)[2], double (*out)[2])
{
    double cur[12][2], nxt[12][2];
    int n = 4;
    for (int i = 0; i < 4; ++i) { cur[i][0] = subject[i][0]; cur[i][1] = subject[i][1]; }
    double ax = clip[3][0], ay = clip[3][1];
    for (int e = 0; e < 4; ++e) {
        const double bx = clip[e][0], by = clip[e][1];
        if (n == 0) return 0;
        const double ex = bx - ax, ey = by - ay;
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int q = (i + n - 1) % n;
            const double sp = ex * (cur[i][1] - ay) - ey * (cur[i][0] - ax);
            const double sq = ex * (cur[q][1] - ay) - ey * (cur[q][0] - ax);
            if ((sp > 0) != (sq > 0)) {
                const double t = sq / (sq - sp);         // opposite signs: never 0/0, always in [0, 1], also when both are rounding noise
                nxt[m][0] = cur[q][0] + t * (cur[i][0] - cur[q][0]);
                nxt[m][1] = cur[q][1] + t * (cur[i][1] - cur[q][1]);
                ++m;
            }
            if (sp > 0) { nxt[m][0] = cur[i][0]; nxt[m][1] = cur[i][1]; ++m; }
        }
        n = m;
        for (int i = 0; i < n; ++i) { cur[i][0] = nxt[i][0]; cur[i][1] = nxt[i][1]; }
        ax = bx; ay = by;
    }
    for (int i = 0; i < n; ++i) { out[i][0] = cur[i][0]; out[i][1] = cur[i][1]; }
    return n;
}

// evalgeom.bev_rect(c[:2], c[3:5], c[6]): counter-clockwise in (x, y)
__device__ void ev_rect(const float *b, double (*rect)[2])
{
    const double cx = b[0], cy = b[1], l = b[3], w = b[4], yaw = b[6];
    const double hl = l / 2, hw = w / 2, c = cos(yaw), s = sin(yaw);
    const double sl[4] = {-1, 1, 1, -1}, sw[4] = {-1, -1, 1, 1};
    for (int k = 0; k < 4; ++k) {
        rect[k][0] = cx + sl[k] * hl * c - sw[k] * hw * s;
        rect[k][1] = cy + sl[k] * hl * s + sw[k] * hw * c;
    }
}

// bird's-eye IoU of two bev_rect rectangles (evalrank.bev_iou): no nudge; NaN for a zero-area pair (compares false everywhere)
__device__ double ev_bev_iou(const double (*r1)[2], const double (*r2)[2])
{
    double poly[12][2];
    const int n = ev_clip(r1, r2, poly);
    const double ia = n >= 3 ? ev_shoelace(poly, n) : 0.0;
    const double a1 = ev_shoelace(r1, 4), a2 = ev_shoelace(r2, 4);
    return ia / (a1 + a2 - ia);
}

}  // namespace
