// fusion_det.hip -- the fusion layer's backward for `deterministic: true`.
// DCF-DETERMINISTIC-SOURCE: tests/test_determinism_host.py scans this file; no float atomics may appear in it.
//
// The default backward sums with fp32 atomics, so the order of the terms -- and with it the last bits of the camera-stream and
// fusion-MLP gradients -- depends on timing.  Here every sum has ONE order that depends on the shapes and the data only:
//   (a) dcf_inv_sort_segments      every segment of an inverse map in ascending key order (the fill's atomic cursor leaves the order
//                                  of a segment to timing; integer atomics are fine for WHERE a segment lies, not for its order)
//   (b) dcf_cam_invert             camera-map pixel -> sorted list of the (point, tap) that touch it (inverse of the bilinear scatter)
//   (c) dcf_point_sample_bwd_det   one wave per camera pixel walks its list and stores the row once (no zero-fill, no atomics)
//   (d) dcf_fusion_gather_bwd_det  slices of 128 pairs per wave as in the default kernel (balanced whatever a point's fan-in); a
//                                  point whose run crosses slices leaves fp32 partial rows indexed by SLICE, added in slice order
//                                  by a second small launch; dW1d / db1 go wave row -> workgroup row -> workspace row, folded
//                                  by k_rows_fold in an association fixed by the row count
//   (e) dcf_rowscale_bias_bwd_det  fc2's bias gradient: workgroup rows + the same fold
// Hand-overs between workgroups are launch boundaries on one stream: no tickets, no fences.
#include <stdlib.h>

#include <algorithm>

#include "dcf_common.h"
#include "fusion_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ (a) segment sort
// Keys are unique inside a segment, so an element's place is the number of smaller keys (rank sort: no exchanges, every element is
// written once).  Four segments per workgroup: a wave sorts a segment of up to 64 keys in registers; longer ones (an isolated far
// point owns thousands of BEV pixels) are taken one after the other by the whole workgroup -- from LDS up to SORT_LDS keys, from a
// copy in `scratch` (same offsets as keys) beyond: quadratic there, but correct.
constexpr int SORT_LDS = 4096;
constexpr int KEY_MAX = 0x7fffffff;

__global__ void __launch_bounds__(256) k_inv_sort_segments(const int *__restrict__ start, int nseg, int *keys, int *scratch)
{
    __shared__ int sk[SORT_LDS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int seg0 = blockIdx.x * 4;
    {
        const int s = seg0 + wv;
        if (s < nseg) {
            const int rs = __builtin_amdgcn_readfirstlane(start[s]);
            const int L = __builtin_amdgcn_readfirstlane(start[s + 1]) - rs;
            if (L > 1 && L <= 64) {
                const int k = lane < L ? keys[rs + lane] : KEY_MAX;
                int rank = 0;
                for (int i = 0; i < L; ++i) rank += __builtin_amdgcn_readlane(k, i) < k ? 1 : 0;
                if (lane < L) keys[rs + rank] = k;          // every lane's load is behind the readlanes above
            }
        }
    }
    for (int q = 0; q < 4; ++q) {                           // workgroup-uniform control flow from here on
        const int s = seg0 + q;
        if (s >= nseg) break;
        const int rs = start[s], L = start[s + 1] - rs;
        if (L <= 64) continue;
        if (L <= SORT_LDS) {
            const int L4 = (L + 3) & ~3;
            for (int i = threadIdx.x; i < L4; i += blockDim.x) sk[i] = i < L ? keys[rs + i] : KEY_MAX;
            __syncthreads();
            for (int i = threadIdx.x; i < L; i += blockDim.x) {
                const int k = sk[i];
                int rank = 0;
                for (int j = 0; j < L4; j += 4) {
                    const int4 o = *reinterpret_cast<const int4 *>(&sk[j]);
                    rank += (o.x < k ? 1 : 0) + (o.y < k ? 1 : 0) + (o.z < k ? 1 : 0) + (o.w < k ? 1 : 0);
                }
                keys[rs + rank] = k;
            }
            __syncthreads();
        } else {
            for (int i = threadIdx.x; i < L; i += blockDim.x) scratch[rs + i] = keys[rs + i];
            __syncthreads();                                // the copy is read by the other waves of this workgroup only
            for (int i = threadIdx.x; i < L; i += blockDim.x) {
                const int k = scratch[rs + i];
                int rank = 0;
                for (int j = 0; j < L; ++j) rank += scratch[rs + j] < k ? 1 : 0;
                keys[rs + rank] = k;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ (b) camera-pixel map
// Segment (frame b, pixel) = b * (HW + 1) + pixel (one spare slot per frame, as the KNN maps have).  Key = point * 4 + tap: unique
// inside a segment even where the border clamp folds two taps of a point onto one pixel.
__device__ __forceinline__ void tap_pixels(const Taps &t, int Wf, int (&pix)[4])
{
    pix[0] = t.y0 * Wf + t.x0; pix[1] = t.y0 * Wf + t.x1; pix[2] = t.y1 * Wf + t.x0; pix[3] = t.y1 * Wf + t.x1;
}

__global__ void __launch_bounds__(256) k_cam_hist(const float *__restrict__ uv, int64_t uv_fs, const int *__restrict__ count, int n_max, int Hf, int Wf,
                                                  int *cnt)
{
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= min(count[b], n_max)) return;
    const float *q = uv + b * uv_fs + 2 * (int64_t)p;
    int pix[4];
    tap_pixels(make_taps(q[0], q[1], Hf, Wf), Wf, pix);
    int *c = cnt + (int64_t)b * (Hf * Wf + 1);
#pragma unroll
    for (int t = 0; t < 4; ++t) atomicAdd(&c[pix[t]], 1);
}

__global__ void __launch_bounds__(256) k_cam_fill(const float *__restrict__ uv, int64_t uv_fs, const int *__restrict__ count, int n_max, int Hf, int Wf,
                                                  int *cursor, int *ent)
{
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= min(count[b], n_max)) return;
    const float *q = uv + b * uv_fs + 2 * (int64_t)p;
    int pix[4];
    tap_pixels(make_taps(q[0], q[1], Hf, Wf), Wf, pix);
    int *c = cursor + (int64_t)b * (Hf * Wf + 1);
#pragma unroll
    for (int t = 0; t < 4; ++t) ent[atomicAdd(&c[pix[t]], 1)] = p * 4 + t;      // (integer cursor: the sort fixes the order)
}

// exclusive scan of n counts by ONE workgroup (n = B * (HW + 1), some 1e4 .. 1e5): thread t owns a contiguous chunk
__global__ void __launch_bounds__(1024) k_scan_counts(const int *__restrict__ cnt, int n, int *start, int *cursor)
{
    __shared__ int tot[1024];
    const int per = (n + 1023) / 1024;
    const int lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += cnt[i];
    tot[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                    // Hillis-Steele over the 1024 chunk sums
        const int v = (int)threadIdx.x >= o ? tot[threadIdx.x - o] : 0;
        __syncthreads();
        tot[threadIdx.x] += v;
        __syncthreads();
    }
    int run = tot[threadIdx.x] - s;
    for (int i = lo; i < hi; ++i) {
        const int c = cnt[i];
        start[i] = run; cursor[i] = run;
        run += c;
    }
}

// ------------------------------------------------------------------------------------------------ (c) point-sample backward
// One wave per camera-map pixel, lane = channel (+ 64 j).  The wave prepares 64 list entries at a time lane-parallel (point row,
// tap weight recomputed from uv) and then walks them in list order: acc += g[point] * weight, the products and the order of the
// additions fixed by the sorted list.  The row is stored once; a pixel nobody touches stores zeros.
template <typename T, int CJ>
__global__ void __launch_bounds__(256) k_point_sample_bwd_det(const T *__restrict__ gfp, int Hf, int Wf, const float *__restrict__ uv,
                                                              const int *__restrict__ start, const int *__restrict__ ent, float *__restrict__ gfmap,
                                                              FrameStride fs)
{
    constexpr int C = 64 * CJ, U = 4;
    const int HW = Hf * Wf;
    const int lane = threadIdx.x & 63;
    const int pix = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (pix >= HW) return;
    gfp += blockIdx.y * fs.a; uv += blockIdx.y * fs.b; gfmap += blockIdx.y * fs.d;
    const int *seg = start + (int64_t)blockIdx.y * (HW + 1);
    const int rs = __builtin_amdgcn_readfirstlane(seg[pix]), re = __builtin_amdgcn_readfirstlane(seg[pix + 1]);
    float acc[CJ];
#pragma unroll
    for (int j = 0; j < CJ; ++j) acc[j] = 0.f;
    for (int base = rs; base < re; base += 64) {
        const int n = min(64, re - base);
        const int key = lane < n ? ent[base + lane] : 0;
        const int p = key >> 2, tap = key & 3;
        const Taps t = make_taps(uv[2 * p], uv[2 * p + 1], Hf, Wf);
        const float l_w = tap == 0 ? t.w00 : (tap == 1 ? t.w01 : (tap == 2 ? t.w10 : t.w11));
        const int l_row = p * C;
        for (int i0 = 0; i0 < n; i0 += U) {
            float g[U][CJ], w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = min(i0 + u, n - 1);           // past the end: a harmless re-read, skipped below
                const int row = __builtin_amdgcn_readlane(l_row, i);
                w[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l_w), i));
#pragma unroll
                for (int j = 0; j < CJ; ++j) g[u][j] = DT<T>::ld(gfp + row + lane + 64 * j);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (i0 + u >= n) break;
#pragma unroll
                for (int j = 0; j < CJ; ++j) acc[j] += g[u][j] * w[u];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < CJ; ++j) gfmap[(int64_t)pix * C + lane + 64 * j] = acc[j];
}

// ------------------------------------------------------------------------------------------------ (d) fusion gather backward
constexpr int FGD_THREADS = 1024;

// part: [frame][slice][2][C] fp32 -- row 0 = the piece of the slice's FIRST point when that point's run began in an earlier slice or
// goes on into the next; row 1 = the piece of its LAST point when the run goes on and the point is not also the first.
// wpart: [frame][workgroup][4 C] -- the workgroup's dW1d (x3) / db1 sums.
template <typename T, int CJ>
__global__ void __launch_bounds__(CJ >= 4 ? FGD_THREADS / 2 : FGD_THREADS) k_fusion_gather_bwd_det(
    const T *__restrict__ P, const float *__restrict__ xyz, const int *__restrict__ e_begin, int n_max, const int *__restrict__ ent_pix,
    const int *__restrict__ ent_pt, FuseGeom g, const float *__restrict__ w1d, const float *__restrict__ b1, const T *__restrict__ ghsum,
    T *__restrict__ gP, float *__restrict__ part, float *__restrict__ wpart, int SL, int nslices, FrameStride fs)
{
    constexpr int C = 64 * CJ, U = 8;
    P += blockIdx.y * fs.a; gP += blockIdx.y * fs.a; xyz += blockIdx.y * fs.b; e_begin += blockIdx.y * fs.c; ghsum += blockIdx.y * fs.d;
    part += (size_t)blockIdx.y * nslices * 2 * C;
    extern __shared__ float sm[];                           // [waves][C][4]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + wv);
    const int nwaves = gridDim.x * (blockDim.x >> 6);       // the grid depends on the shapes only: a wave takes slices wave, wave + nwaves, ...
    const int E0 = e_begin[0], E = e_begin[n_max];
    float w0[CJ], w1[CJ], w2[CJ], bb[CJ], a0[CJ], a1[CJ], a2[CJ], ab[CJ], cur_acc[CJ];
#pragma unroll
    for (int j = 0; j < CJ; ++j) {
        const int c = lane + 64 * j;
        w0[j] = w1d[c * 3]; w1[j] = w1d[c * 3 + 1]; w2[j] = w1d[c * 3 + 2]; bb[j] = b1[c];
        a0[j] = a1[j] = a2[j] = ab[j] = cur_acc[j] = 0.f;
    }
    auto bcast_i = [](int v, int i) { return __builtin_amdgcn_readlane(v, i); };
    auto bcast_f = [](float v, int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i)); };
    for (int sidx = wave; sidx < nslices && E0 + sidx * SL < E; sidx += nwaves) {
        const int lo = E0 + sidx * SL, hi = min(E, lo + SL);
        bool open_left = lo > E0 && ent_pt[lo - 1] == ent_pt[lo];      // the slice's first point began in an earlier slice
        bool is_first = true;
        int cur_pt = -1;
        auto flush = [&](bool open) {                       // open: the point has pairs outside this slice
            if (open) {
                float *row = part + ((size_t)sidx * 2 + (is_first ? 0 : 1)) * C;
#pragma unroll
                for (int j = 0; j < CJ; ++j) row[lane + 64 * j] = cur_acc[j];
            } else {
#pragma unroll
                for (int j = 0; j < CJ; ++j) DT<T>::st(gP + (int64_t)cur_pt * C + lane + 64 * j, cur_acc[j]);
            }
        };
        for (int base = lo; base < hi; base += 64) {
            const int n = min(64, hi - base);
            // lane-parallel preparation of 64 pairs: pixel centre (IEEE division once per pair), offsets to the point, row offsets
            const bool live = lane < n;
            const int l_pix = live ? ent_pix[base + lane] : 0;
            const int l_pt = live ? ent_pt[base + lane] : 0;
            const int pi = l_pix >> 16, pj = l_pix & 0xffff;
            float Xc, Yc;
            pixel_centre(g, pi, pj, Xc, Yc);
            const float l_dx = xyz[3 * l_pt] - Xc, l_dy = xyz[3 * l_pt + 1] - Yc, l_dz = xyz[3 * l_pt + 2];
            const int l_grow = (pi * g.w + pj) * C, l_prow = l_pt * C;
            for (int i0 = 0; i0 < n; i0 += U) {
                int pt[U];
                float dx[U], dy[U], dz[U], gg[U][CJ], pv[U][CJ];
#pragma unroll
                for (int u = 0; u < U; ++u) {               // issue every load of the group first
                    const int i = min(i0 + u, n - 1);        // past the end: a harmless re-read, skipped below
                    pt[u] = bcast_i(l_pt, i);
                    dx[u] = bcast_f(l_dx, i); dy[u] = bcast_f(l_dy, i); dz[u] = bcast_f(l_dz, i);
                    const int grow = bcast_i(l_grow, i), prow = bcast_i(l_prow, i);
#pragma unroll
                    for (int j = 0; j < CJ; ++j) {
                        gg[u][j] = DT<T>::ld(ghsum + grow + lane + 64 * j);
                        pv[u][j] = DT<T>::ld(P + prow + lane + 64 * j);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (i0 + u >= n) break;
                    if (pt[u] != cur_pt) {                   // wave-uniform
                        if (cur_pt >= 0) {
                            flush(is_first && open_left);    // a point that ends inside the slice is open on its left side at most
                            is_first = false;
                        }
                        cur_pt = pt[u];
#pragma unroll
                        for (int j = 0; j < CJ; ++j) cur_acc[j] = 0.f;
                    }
#pragma unroll
                    for (int j = 0; j < CJ; ++j) {
                        const float pre = pv[u][j] + (w0[j] * dx[u] + w1[j] * dy[u] + w2[j] * dz[u]) + bb[j];
                        const float d = pre > 0.f ? gg[u][j] : 0.f;
                        cur_acc[j] += d;
                        a0[j] += d * dx[u]; a1[j] += d * dy[u]; a2[j] += d * dz[u]; ab[j] += d;
                    }
                }
            }
        }
        if (cur_pt >= 0) {
            const bool open_right = hi < E && ent_pt[hi] == cur_pt;
            flush((is_first && open_left) || open_right);
        }
#pragma unroll
        for (int j = 0; j < CJ; ++j) cur_acc[j] = 0.f;
    }
    // dW1d / db1: the wave's sums to its own LDS row, the workgroup's rows added in wave order, the result to the workgroup's row
    float *mine = sm + (size_t)wv * 4 * C;
#pragma unroll
    for (int j = 0; j < CJ; ++j) {
        const int c = lane + 64 * j;
        mine[c * 4 + 0] = a0[j]; mine[c * 4 + 1] = a1[j]; mine[c * 4 + 2] = a2[j]; mine[c * 4 + 3] = ab[j];
    }
    __syncthreads();
    const int nw = blockDim.x >> 6;
    float *out = wpart + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 * C;
    for (int i = threadIdx.x; i < 4 * C; i += blockDim.x) {
        float tot = 0.f;
        for (int q = 0; q < nw; ++q) tot += sm[(size_t)q * 4 * C + i];
        out[i] = tot;
    }
}

// Second launch of (d): one wave per point row -- a point without pairs stores zeros, a point whose run crosses slices adds its
// partial rows in slice order and stores the sum, any other row was stored whole by the first launch.  (The workgroups' dW1d / db1
// rows are folded onto the gradient arena by k_rows_fold<true>, a third small launch.)
template <typename T, int CJ>
__global__ void __launch_bounds__(256) k_fusion_gather_bwd_det_fin(const int *__restrict__ e_begin, int n_rows, T *__restrict__ gP,
                                                                   const float *__restrict__ part, int SL, int nslices, FrameStride fs)
{
    constexpr int C = 64 * CJ;
    gP += blockIdx.y * fs.a; e_begin += blockIdx.y * fs.c;
    part += (size_t)blockIdx.y * nslices * 2 * C;
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (p >= n_rows) return;
    const int E0 = e_begin[0];
    const int rs = __builtin_amdgcn_readfirstlane(e_begin[p] - E0), re = __builtin_amdgcn_readfirstlane(e_begin[p + 1] - E0);
    float tot[CJ];
#pragma unroll
    for (int j = 0; j < CJ; ++j) tot[j] = 0.f;
    if (rs < re) {
        const int s_first = rs / SL, s_last = (re - 1) / SL;
        if (s_first == s_last) return;
        for (int s = s_first; s <= s_last; ++s) {
            const int which = (s == s_first && rs > s * SL) ? 1 : 0;      // the run starts inside its first slice: that slice's last point
            const float *row = part + ((size_t)s * 2 + which) * C;
#pragma unroll
            for (int j = 0; j < CJ; ++j) tot[j] += row[lane + 64 * j];
        }
    }
#pragma unroll
    for (int j = 0; j < CJ; ++j) DT<T>::st(gP + (int64_t)p * C + lane + 64 * j, tot[j]);
}

// ------------------------------------------------------------------------------------------------ (e) fc2 bias gradient
// The streaming pass of k_relu_mask_rowscale_bwd / k_rowscale_bias_bwd (elementwise.hip) with the workgroup's channel sums stored to
// its own workspace row instead of added onto gb2; k_rows_fold adds the rows in workgroup order.
template <typename T, int V>
__device__ __forceinline__ void ldv_(const T *p, float (&v)[V])
{
    if constexpr (V == 8) ld8(p, v);
    else { const float4 t = ld4(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
}
template <typename T, int V>
__device__ __forceinline__ void stv_(T *p, const float (&v)[V])
{
    if constexpr (V == 8) st8(p, v);
    else st4(p, make_float4(v[0], v[1], v[2], v[3]));
}

template <typename T, int V, bool MASK>
__global__ void __launch_bounds__(256) k_rowscale_bias_bwd_det(const T *__restrict__ gy, const T *__restrict__ y, const float *__restrict__ cnt,
                                                               T *__restrict__ gout, float *__restrict__ rows, int64_t nvec, int cgroups, int64_t stride)
{
    extern __shared__ float sm[];  // [256][V]
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float acc[V];
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] = 0.f;
    if (t < stride) {
        int64_t p = t / cgroups;                          // pixel of element e; stride is a multiple of cgroups
        const int64_t pstep = stride / cgroups;
        int64_t e = t;
        for (; e + 3 * stride < nvec; e += 4 * stride, p += 4 * pstep) {
            float g[4][V], yy[4][V], k[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                ldv_<T, V>(gy + (e + u * stride) * V, g[u]);
                if (MASK) ldv_<T, V>(y + (e + u * stride) * V, yy[u]);
                k[u] = cnt[p + u * pstep];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float m[V];
#pragma unroll
                for (int q = 0; q < V; ++q) {
                    acc[q] += k[u] * g[u][q];
                    if (MASK) m[q] = yy[u][q] > 0.f ? g[u][q] : 0.f;
                }
                if (MASK) stv_<T, V>(gout + (e + u * stride) * V, m);
            }
        }
        for (; e < nvec; e += stride, p += pstep) {
            float g[V], yy[V], m[V];
            ldv_<T, V>(gy + e * V, g);
            if (MASK) ldv_<T, V>(y + e * V, yy);
            const float k = cnt[p];
#pragma unroll
            for (int q = 0; q < V; ++q) {
                acc[q] += k * g[q];
                if (MASK) m[q] = yy[q] > 0.f ? g[q] : 0.f;
            }
            if (MASK) stv_<T, V>(gout + e * V, m);
        }
    }
#pragma unroll
    for (int q = 0; q < V; ++q) sm[threadIdx.x * V + q] = acc[q];
    __syncthreads();
    // channel i = group j x lane q of it; the threads of this workgroup whose elements belong to group j: t % cgroups == j
    for (int i = threadIdx.x; i < cgroups * V; i += blockDim.x) {
        const int j = i / V, q = i - j * V;
        const int base = (int)(((int64_t)blockIdx.x * blockDim.x) % cgroups);
        int first = j - base;
        if (first < 0) first += cgroups;
        float sum = 0.f;
        for (int th = first; th < (int)blockDim.x; th += cgroups) sum += sm[th * V + q];
        rows[(size_t)blockIdx.x * cgroups * V + i] = sum;
    }
}

// dst[i] += the sum of column i over the rows, in ONE association fixed by (nrows) alone: 16 threads share a column, thread g adds
// rows g, g + 16, g + 32, ... in that order, then the 16 partial sums are added in thread order.  (One thread per column walking
// 256 rows was one exposed load latency per row: 60 us per launch, 0.7 ms per cfg2 step over the folds of a backward.)
// W1D: the columns are a fusion site's [C][4] sums (dW1d x3, db1): column c*4+q goes to dst[c*3+q] (q < 3) or dst2[c].
template <bool W1D>
__global__ void __launch_bounds__(256) k_rows_fold(const float *__restrict__ rows, int nrows, int n, float *dst, float *dst2)
{
    __shared__ float sm[16][17];
    const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + cl;
    float part = 0.f;
    if (i < n)
        for (int r = g; r < nrows; r += 16) part += rows[(size_t)r * n + i];
    sm[g][cl] = part;
    __syncthreads();
    if (g != 0 || i >= n) return;
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) tot += sm[q][cl];
    if (W1D) {
        const int c = i >> 2, q = i & 3;
        if (q < 3) dst[c * 3 + q] += tot; else dst2[c] += tot;
    } else {
        dst[i] += tot;
    }
}

}  // namespace

// ================================================================== C ABI
extern "C" int dcf_inv_sort_segments(const int32_t *start, int nseg, int32_t *keys, int32_t *scratch, dcf_stream_t stream)
{
    DCF_REQUIRE(start && keys && scratch && nseg >= 0, "dcf_inv_sort_segments: bad arguments");
    if (nseg == 0) return DCF_OK;
    hipStream_t s = S(stream);
    DCF_LAUNCH("inv_sort_segments", s, hipLaunchKernelGGL(k_inv_sort_segments, dim3(cdiv(nseg, 4)), dim3(256), 0, s, start, nseg, keys, scratch));
    return DCF_OK;
}

extern "C" size_t dcf_cam_invert_workspace_bytes(int Hf, int Wf, int B) { return sizeof(int) * 2 * (size_t)B * ((size_t)Hf * Wf + 1); }

extern "C" int dcf_cam_invert(const float *uv, int64_t uv_fstride, const int32_t *count_dev, int n_max, int Hf, int Wf, int B, int32_t *start,
                              int32_t *ent, int32_t *scratch, void *ws, dcf_stream_t stream)
{
    DCF_REQUIRE(uv && count_dev && start && ent && scratch && ws && Hf >= 1 && Wf >= 1 && B >= 1 && B <= 65535 && n_max >= 0,
                "dcf_cam_invert: bad arguments");
    DCF_REQUIRE((int64_t)n_max * 4 < (1ll << 31) / std::max(B, 1) && (int64_t)B * ((int64_t)Hf * Wf + 1) < (1ll << 31), "dcf_cam_invert: too many entries");
    hipStream_t s = S(stream);
    const int nscan = B * (Hf * Wf + 1);
    int *cnt = (int *)ws, *cursor = cnt + nscan;
    DCF_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)nscan, s));
    if (n_max > 0) DCF_LAUNCH_B("cam_hist", (double)B * n_max * 24.0, s, hipLaunchKernelGGL(k_cam_hist, dim3(cdiv(n_max, 256), B), dim3(256), 0, s, uv, uv_fstride, count_dev, n_max, Hf, Wf, cnt));
    DCF_LAUNCH("cam_scan", s, hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, cnt, nscan, start, cursor));
    if (n_max > 0) {
        DCF_LAUNCH_B("cam_fill", (double)B * n_max * 40.0, s, hipLaunchKernelGGL(k_cam_fill, dim3(cdiv(n_max, 256), B), dim3(256), 0, s, uv, uv_fstride, count_dev, n_max, Hf, Wf, cursor, ent));
        DCF_LAUNCH("cam_sort_segments", s, hipLaunchKernelGGL(k_inv_sort_segments, dim3(cdiv(nscan - 1, 4)), dim3(256), 0, s, start, nscan - 1, ent, scratch));
    }
    return DCF_OK;
}

extern "C" int dcf_point_sample_bwd_det(int dtype, const void *gfp, int64_t gfp_rows, int Hf, int Wf, int Cf, const float *uv, int64_t uv_fstride,
                                        const int32_t *start, const int32_t *ent, float *gfmap, int B, dcf_stream_t stream)
{
    DCF_REQUIRE(gfp && uv && start && ent && gfmap && B >= 1 && B <= 65535 && Hf >= 1 && Wf >= 1, "dcf_point_sample_bwd_det: bad arguments");
    DCF_REQUIRE(Cf % 64 == 0 && Cf >= 64 && Cf <= 256, "dcf_point_sample_bwd_det: Cf must be 64, 128, 192 or 256 (got %d)", Cf);
    hipStream_t s = S(stream);
    const int HW = Hf * Wf;
    const FrameStride fs = {gfp_rows * Cf, uv_fstride, 0, (int64_t)HW * Cf, 0};
#define DCF_PSD(CJ_) DCF_LAUNCH_B("point_sample_bwd_det", (double)B * (HW * (Cf * 4.0 + 4.0) + gfp_rows * (4.0 * Cf * sizeof(T) + 24.0)), s, hipLaunchKernelGGL((k_point_sample_bwd_det<T, CJ_>), dim3(cdiv(HW, 4), B), dim3(256), 0, s, (const T *)gfp, Hf, Wf, uv, start, ent, gfmap, fs))
    DCF_DISPATCH_DTYPE(dtype, {
        if (Cf == 64) DCF_PSD(1);
        else if (Cf == 128) DCF_PSD(2);
        else if (Cf == 192) DCF_PSD(3);
        else DCF_PSD(4);
    })
#undef DCF_PSD
    return DCF_OK;
}

// pairs per wave, as the default kernel chooses them
static int fgd_slice(int max_entries)
{
    int sl = cdiv(cdiv(max_entries, 4096), 16) * 16;
    return sl < 16 ? 16 : (sl > 128 ? 128 : sl);
}
static int fgd_threads(int Cb) { return Cb >= 256 ? FGD_THREADS / 2 : FGD_THREADS; }
static int fgd_blocks(int max_entries, int Cb, int B)
{
    const int waves = cdiv(max_entries, fgd_slice(max_entries));
    return std::max(1, std::min(cdiv(waves, fgd_threads(Cb) / 64), std::max(256 / B, 32)));
}

// floats: [B][slices][2][Cb] partial point rows, then [B][workgroups][4 Cb] dW1d / db1 rows.  Nothing has to be zeroed.
extern "C" size_t dcf_fusion_gather_bwd_det_workspace_bytes(int max_entries, int Cb, int B)
{
    if (max_entries <= 0 || B <= 0) return 0;
    const size_t slices = cdiv(max_entries, fgd_slice(max_entries));
    return sizeof(float) * ((size_t)B * slices * 2 * Cb + (size_t)B * fgd_blocks(max_entries, Cb, B) * 4 * Cb);
}

extern "C" int dcf_fusion_gather_bwd_det(int dtype, const void *P, int64_t p_rows, const float *xyz, int64_t xyz_fstride, const int32_t *start,
                                         int n_max, const int32_t *ent_pix, const int32_t *ent_pt, int max_entries, int h, int w, int stride,
                                         float xs, float xo, float ys, float yo, const float *w1d, const float *b1, int Cb, const void *ghsum,
                                         void *gP, float *gw1d, float *gb1, void *workspace, int B, dcf_stream_t stream)
{
    DCF_REQUIRE(P && xyz && start && ent_pix && ent_pt && w1d && b1 && ghsum && gP && gw1d && gb1 && workspace, "dcf_fusion_gather_bwd_det: null pointer");
    DCF_REQUIRE(Cb % 64 == 0 && Cb >= 64 && Cb <= 256, "dcf_fusion_gather_bwd_det: Cb must be 64, 128, 192 or 256 (got %d)", Cb);
    DCF_REQUIRE(B >= 1 && B <= 64 && p_rows >= 0 && p_rows <= n_max && max_entries > 0, "dcf_fusion_gather_bwd_det: 1..64 frames, p_rows <= n_max, max_entries > 0");
    FuseGeom g;
    g.h = h; g.w = w; g.stride = stride; g.K = 0; g.xs = xs; g.xo = xo; g.ys = ys; g.yo = yo;
    hipStream_t s = S(stream);
    const int sl = fgd_slice(max_entries), nslices = cdiv(max_entries, sl), thr = fgd_threads(Cb), blocks = fgd_blocks(max_entries, Cb, B);
    float *part = reinterpret_cast<float *>(workspace);
    float *wpart = part + (size_t)B * nslices * 2 * Cb;
    const FrameStride fs = {p_rows * Cb, xyz_fstride, (int64_t)n_max + 1, (int64_t)h * w * Cb, 0};
    const int rows = (int)p_rows;
#define DCF_FGD(CJ_)                                                                                                                                  \
    do {                                                                                                                                              \
        DCF_LAUNCH_B("fusion_gather_bwd_det<" #CJ_ ">", (double)B * max_entries * (8.0 + 2.0 * Cb * sizeof(T)), s,                                    \
                     hipLaunchKernelGGL((k_fusion_gather_bwd_det<T, CJ_>), dim3(blocks, B), dim3(thr), sizeof(float) * (thr / 64) * 4 * Cb, s,         \
                                        (const T *)P, xyz, start, n_max, ent_pix, ent_pt, g, w1d, b1, (const T *)ghsum, (T *)gP, part, wpart, sl,      \
                                        nslices, fs));                                                                                                \
        DCF_LAUNCH_B("fusion_gather_bwd_det_fin", (double)B * rows * Cb * sizeof(T), s,                                                               \
                     hipLaunchKernelGGL((k_fusion_gather_bwd_det_fin<T, CJ_>), dim3(std::max(cdiv(rows, 4), 1), B), dim3(256), 0, s, start, rows,       \
                                        (T *)gP, part, sl, nslices, fs));                                                                             \
    } while (0)
    DCF_DISPATCH_DTYPE(dtype, {
        if (Cb == 64) DCF_FGD(1);
        else if (Cb == 128) DCF_FGD(2);
        else if (Cb == 192) DCF_FGD(3);
        else DCF_FGD(4);
    })
#undef DCF_FGD
    DCF_LAUNCH("fusion_gather_bwd_det_fold", s, hipLaunchKernelGGL(k_rows_fold<true>, dim3(cdiv(4 * Cb, 16)), dim3(256), 0, s, wpart, B * blocks, 4 * Cb, gw1d, gb1));
    return DCF_OK;
}

static int64_t det_chan_stride(int64_t nvec, int cgroups, int &blocks)
{
    const int64_t cap = 64 * 1024ll;                       // <= 256 workgroups: the rows the fold walks
    int64_t want = nvec < cap ? nvec : cap;
    if (want < cgroups) want = cgroups;
    const int64_t stride = want / cgroups * cgroups;
    blocks = cdiv(stride, 256);
    return stride;
}

extern "C" size_t dcf_rowscale_bias_bwd_det_workspace_bytes(int C) { return sizeof(float) * 256 * (size_t)C; }

// gb2[c] += sum_p cnt[p] * gy[p][c] in one fixed order; y / gout both null (the bias gradient alone) or both given (gout = gy * (y > 0)
// as dcf_relu_mask_rowscale_bwd writes it).
extern "C" int dcf_rowscale_bias_bwd_det(int dtype, const void *gy, const void *y, const float *cnt, void *gout, float *gb2, int64_t npix, int C,
                                         void *workspace, dcf_stream_t stream)
{
    DCF_REQUIRE(gy && cnt && gb2 && workspace && C % 4 == 0 && (y == nullptr) == (gout == nullptr) && (gout == nullptr || gout != gy),
                "dcf_rowscale_bias_bwd_det: bad arguments (y and gout come together; gout must be its own tensor)");
    const int V = C % 8 == 0 ? 8 : 4;
    const int cg = C / V;
    const int64_t nvec = npix * cg;
    if (nvec == 0) return DCF_OK;
    int blocks;
    const int64_t stride = det_chan_stride(nvec, cg, blocks);
    float *rows = reinterpret_cast<float *>(workspace);
    hipStream_t s = S(stream);
#define DCF_RBD(V_, M_) DCF_LAUNCH_B(M_ ? "relu_mask_rowscale_bwd_det" : "rowscale_bias_bwd_det", bytes, s, hipLaunchKernelGGL((k_rowscale_bias_bwd_det<T, V_, M_>), dim3(blocks), dim3(256), sizeof(float) * 256 * V_, s, (const T *)gy, (const T *)y, cnt, (T *)gout, rows, nvec, cg, stride))
    DCF_DISPATCH_DTYPE(dtype, {
        const double bytes = (double)npix * C * sizeof(T) * (y ? 3 : 1) + npix * 4.0;
        if (V == 8) { if (y) DCF_RBD(8, true); else DCF_RBD(8, false); }
        else { if (y) DCF_RBD(4, true); else DCF_RBD(4, false); }
    })
#undef DCF_RBD
    DCF_LAUNCH("rows_fold", s, hipLaunchKernelGGL(k_rows_fold<false>, dim3(cdiv(C, 16)), dim3(256), 0, s, rows, blocks, C, gb2, (float *)nullptr));
    return DCF_OK;
}

// *dst += rows[0] + rows[1] + ... (the loss kernels' per-sample values: see loss.hip)
extern "C" int dcf_rows_fold(const float *rows, int nrows, int n, float *dst, dcf_stream_t stream)
{
    DCF_REQUIRE(rows && dst && nrows >= 0 && n >= 1, "dcf_rows_fold: bad arguments");
    hipStream_t s = S(stream);
    DCF_LAUNCH("rows_fold", s, hipLaunchKernelGGL(k_rows_fold<false>, dim3(cdiv(n, 16)), dim3(256), 0, s, rows, nrows, n, dst, (float *)nullptr));
    return DCF_OK;
}
