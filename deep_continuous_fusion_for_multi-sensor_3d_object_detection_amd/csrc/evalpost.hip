// evalpost.hip -- evaluation post-processing on the device: what /root/reference/test.py:88-206 does
// with Python loops over boxes on the host -- score threshold + compaction (:88-108), greedy rotated-box suppression in
// input order with the separating-axis test (:142-175) or the 3-D IoU (:110-140), and the bird's-eye-IoU matching behind
// the precision / recall counters (:177-206).  Geometry in fp64 like the host statement (evalgeom.py), decisions
// bit-for-bit the same on tests/golden/eval.npz (survivor indices, TP counters).
//
// Suppression is sequential by definition (a box survives iff it overlaps none of the EARLIER SURVIVORS); here the n^2
// pairwise tests run in parallel into a bit matrix, and one wave (lane = 64-box word of the survivor set) walks the rows.
// HBM traffic is negligible (n <= 4096 boxes): these kernels are latency-bound by design, not on the train-step path.
#include "dcf_common.h"
#include "ev_geom.h"      // ev_shoelace, ev_clip, ev_rect, ev_bev_iou

namespace {

constexpr int EV_CAP = 4096;            // boxes per sample the suppression handles (64 words x 64 bits)

struct EvGeom {                          // per box, computed once
    double rect[4][2];                   // SAT: bird's-eye rectangle in (x, y), size[0] along the heading
    double foot[4][2];                   // IoU: footprint in (x, z), corners 3,2,1,0 of the 8-corner box
    double footn[4][2];                  // the same for the centre nudged by +1e-4 (the survivor's role in NMS_IOU)
    double top, bot, topn, botn;         // y extent (corner 0 / corner 4), plain and nudged
    double area, vol, arean, voln;       // footprint area and box volume, plain and nudged (equal up to rounding)
};

__device__ void ev_corners(double cx, double cy, double cz, double l, double w, double h, double yaw, double (&X)[8], double (&Y)[8], double (&Z)[8])
{
    const double c = cos(yaw), s = sin(yaw);
    const double sgx[8] = {1, 1, -1, -1, 1, 1, -1, -1}, sgy[8] = {1, 1, 1, 1, -1, -1, -1, -1}, sgz[8] = {1, -1, -1, 1, 1, -1, -1, 1};
    for (int i = 0; i < 8; ++i) {
        const double sx = sgx[i] * (l / 2), sy = sgy[i] * (h / 2), sz = sgz[i] * (w / 2);
        X[i] = c * sx + s * sz + cx;
        Y[i] = sy + cy;
        Z[i] = -s * sx + c * sz + cz;
    }
}

// (3-D IoU, bird's-eye IoU) of a candidate (subject) against a survivor / reference (clip): evalgeom.rotated_iou
__device__ void ev_iou(const double (*f1)[2], double top1, double bot1, double a1, double v1, const double (*f2)[2], double top2, double bot2,
                       double a2, double v2, double &iou3d, double &iou2d)
{
    double poly[12][2];
    const int n = ev_clip(f1, f2, poly);
    const double ia = n >= 3 ? ev_shoelace(poly, n) : 0.0;
    iou2d = ia / (a1 + a2 - ia);
    const double top = fmin(top1, top2), bot = fmax(bot1, bot2);
    const double iv = ia * fmax(0.0, top - bot);
    iou3d = iv / (v1 + v2 - iv);
}

__device__ bool ev_sat(const double (*A)[2], const double (*B)[2])
{
    for (int which = 0; which < 2; ++which) {
        const double (*P)[2] = which == 0 ? A : B;
        for (int i = 0; i < 4; ++i) {
            const int j = (i + 1) & 3;
            const double ex = P[j][0] - P[i][0], ey = P[j][1] - P[i][1];
            double nx = ey, ny = -ex;
            const double norm = hypot(nx, ny);
            nx /= norm; ny /= norm;
            double amin = 1e300, amax = -1e300, bmin = 1e300, bmax = -1e300;
            for (int k = 0; k < 4; ++k) {
                const double pa = A[k][0] * nx + A[k][1] * ny, pb = B[k][0] * nx + B[k][1] * ny;
                amin = fmin(amin, pa); amax = fmax(amax, pa); bmin = fmin(bmin, pb); bmax = fmax(bmax, pb);
            }
            if (amax < bmin || bmax < amin) return false;
        }
    }
    return true;
}

__device__ void ev_prep_one(const float *b, EvGeom &g)
{
    const double cx = b[0], cy = b[1], cz = b[2], l = b[3], w = b[4], h = b[5], yaw = b[6];
    ev_rect(b, g.rect);
    double X[8], Y[8], Z[8];
    ev_corners(cx, cy, cz, l, w, h, yaw, X, Y, Z);
    const int order[4] = {3, 2, 1, 0};
    for (int k = 0; k < 4; ++k) { g.foot[k][0] = X[order[k]]; g.foot[k][1] = Z[order[k]]; }
    g.top = Y[0]; g.bot = Y[4];
    g.area = ev_shoelace(g.foot, 4);
    auto volume = [&]() {
        const double d01 = sqrt((X[0] - X[1]) * (X[0] - X[1]) + (Y[0] - Y[1]) * (Y[0] - Y[1]) + (Z[0] - Z[1]) * (Z[0] - Z[1]));
        const double d12 = sqrt((X[1] - X[2]) * (X[1] - X[2]) + (Y[1] - Y[2]) * (Y[1] - Y[2]) + (Z[1] - Z[2]) * (Z[1] - Z[2]));
        const double d04 = sqrt((X[0] - X[4]) * (X[0] - X[4]) + (Y[0] - Y[4]) * (Y[0] - Y[4]) + (Z[0] - Z[4]) * (Z[0] - Z[4]));
        return d01 * d12 * d04;
    };
    g.vol = volume();
    ev_corners(cx + 0.0001, cy + 0.0001, cz + 0.0001, l, w, h, yaw, X, Y, Z);
    for (int k = 0; k < 4; ++k) { g.footn[k][0] = X[order[k]]; g.footn[k][1] = Z[order[k]]; }
    g.topn = Y[0]; g.botn = Y[4];
    g.arean = ev_shoelace(g.footn, 4);
    g.voln = volume();
}

__global__ void __launch_bounds__(256) k_eval_prep(const float *boxes, const int *count, int n_max, EvGeom *geom)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = count ? min(*count, n_max) : n_max;
    if (i >= n) return;
    ev_prep_one(boxes + (size_t)i * 7, geom[i]);
}

// bit j of mask[i][j / 64] = box i (the candidate) overlaps box j < i (a possible survivor)
__global__ void __launch_bounds__(256) k_eval_pairs(const EvGeom *geom, const int *count, int n_max, int mode, double thr, int words, unsigned long long *mask)
{
    const int n = count ? min(*count, n_max) : n_max;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = t / words, wd = t - i * words;
    if (i >= n) return;
    unsigned long long bits = 0;
    const int j0 = wd * 64;
    if (j0 < i) {
        const EvGeom &gi = geom[i];
        for (int b = 0; b < 64; ++b) {
            const int j = j0 + b;
            if (j >= i) break;
            const EvGeom &gj = geom[j];
            bool over;
            if (mode == 0) {
                over = ev_sat(gi.rect, gj.rect);
            } else if (mode == 2) {
                over = ev_bev_iou(gi.rect, gj.rect) > thr;
            } else {
                double i3, i2;
                ev_iou(gi.foot, gi.top, gi.bot, gi.area, gi.vol, gj.footn, gj.topn, gj.botn, gj.arean, gj.voln, i3, i2);
                over = i3 > thr;
            }
            if (over) bits |= 1ull << b;
        }
    }
    mask[(size_t)i * words + wd] = bits;
}

// one wave: lane = word of the survivor bit set; rows are prefetched 8 ahead (their loads do not depend on the decisions)
__global__ void __launch_bounds__(64) k_eval_scan(const unsigned long long *mask, const int *count, int n_max, int words, int32_t *keep, int32_t *nkeep)
{
    const int n = count ? min(*count, n_max) : n_max;
    const int lane = threadIdx.x;
    unsigned long long kept = 0;
    int total = 0;
    constexpr int U = 8;
    for (int i0 = 0; i0 < n; i0 += U) {
        unsigned long long row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) row[u] = (i0 + u < n && lane < words) ? mask[(size_t)(i0 + u) * words + lane] : 0ull;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u;
            if (i >= n) break;
            const bool hit = (row[u] & kept) != 0ull;
            const bool any = __ballot(hit) != 0ull;
            if (!any) {
                if (lane == (i >> 6)) kept |= 1ull << (i & 63);
                ++total;
            }
            if (lane == 0) keep[i] = any ? 0 : 1;
        }
    }
    if (lane == 0) *nkeep = total;
}

// one thread per kept prediction: OR over the labelled boxes of (bird's-eye IoU > t) per threshold (test.py:190-203)
__global__ void __launch_bounds__(256) k_eval_match(const float *pred, int npred, const float *refs, int nref_rows, const double *thr, int nthr, int32_t *tp)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npred) return;
    EvGeom gp;
    ev_prep_one(pred + (size_t)i * 7, gp);
    unsigned flags = 0;
    for (int r = 0; r < nref_rows; ++r) {
        const float *rb = refs + (size_t)r * 9;
        if (rb[8] != 1.0f) continue;
        EvGeom gr;
        ev_prep_one(rb, gr);
        double i3, i2;
        ev_iou(gp.foot, gp.top, gp.bot, gp.area, gp.vol, gr.foot, gr.top, gr.bot, gr.area, gr.vol, i3, i2);
        for (int t = 0; t < nthr; ++t)
            if (i2 > thr[t]) flags |= 1u << t;
    }
    for (int t = 0; t < nthr; ++t)
        if (flags & (1u << t)) atomicAdd(&tp[t], 1);
}

// Score threshold + order-preserving compaction of one sample per workgroup (test.py:88-108): anchor 0's pixels in raster
// order, then anchor 1's.  pred [B][32][hw] fp32: class scores in channels 2a+1, decoded boxes in channels 18+7a .. +6.
__global__ void __launch_bounds__(1024) k_eval_score_filter(const float *pred, int hw, float thr, int cap, float *boxes, int32_t *count)
{
    __shared__ int wsum[16];
    __shared__ int base_s;
    const int b = blockIdx.x;
    const float *p = pred + (size_t)b * 32 * hw;
    float *out = boxes + (size_t)b * cap * 7;
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c0 = 0; c0 < 2 * hw; c0 += 1024) {
        const int c = c0 + threadIdx.x;
        const int a = c >= hw ? 1 : 0, px = c - a * hw;
        const bool ok = c < 2 * hw && p[(size_t)(2 * a + 1) * hw + px] > thr;
        const unsigned long long bal = __ballot(ok);
        const int before = __popcll(bal & ((1ull << lane) - 1));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = base_s;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        const int pos = off + before;
        if (ok && pos < cap)
            for (int k = 0; k < 7; ++k) out[(size_t)pos * 7 + k] = p[(size_t)(18 + 7 * a + k) * hw + px];
        __syncthreads();
        if (threadIdx.x == 0) { int tot = 0; for (int w = 0; w < 16; ++w) tot += wsum[w]; base_s += tot; }
        __syncthreads();
    }
    if (threadIdx.x == 0) count[b] = base_s;          // may exceed cap: the caller checks
}

// ------------------------------------------------------------------ ranked evaluation (eval_metric: ranked)
// Everything below is decided on integer keys and fp64 geometry (evalrank.py is the host statement).

constexpr int EV_TILE = 1024;            // keys per LDS tile of the counting rank (8 KiB)
constexpr int EV_LEVELS = 40;            // recall levels of the KITTI R40 average precision

// total-order map of fp32 bits: larger float <=> larger unsigned (-0.0 below +0.0)
__device__ __forceinline__ unsigned ev_orderable(float s)
{
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long ev_key(float s, unsigned index)
{
    return ((unsigned long long)ev_orderable(s) << 32) | (unsigned long long)(0xFFFFFFFFu - index);
}

// Keys of one sample's candidates with score > thr, compacted in candidate-index order (one workgroup per sample, as
// k_eval_score_filter).  keys [B][2 hw]; total[b] = how many were kept, count[b] = min(total, cap).
__global__ void __launch_bounds__(1024) k_rank_compact(const float *pred, int hw, float thr, int cap, unsigned long long *keys, int32_t *count, int32_t *total)
{
    __shared__ int wsum[16];
    __shared__ int base_s;
    const int b = blockIdx.x;
    const float *p = pred + (size_t)b * 32 * hw;
    unsigned long long *out = keys + (size_t)b * 2 * hw;
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c0 = 0; c0 < 2 * hw; c0 += 1024) {
        const int c = c0 + threadIdx.x;
        const int a = c >= hw ? 1 : 0, px = c - a * hw;
        const float sc = c < 2 * hw ? p[(size_t)(2 * a + 1) * hw + px] : 0.0f;
        const bool ok = c < 2 * hw && sc > thr;                  // a NaN score is never kept
        const unsigned long long bal = __ballot(ok);
        const int before = __popcll(bal & ((1ull << lane) - 1));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = base_s;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        const int pos = off + before;
        if (ok && pos < 2 * hw) out[pos] = ev_key(sc, (unsigned)c);
        __syncthreads();
        if (threadIdx.x == 0) { int tot = 0; for (int w = 0; w < 16; ++w) tot += wsum[w]; base_s += tot; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { total[b] = base_s; count[b] = min(base_s, cap); }
}

// Rank by counting: the position of a candidate is the number of larger keys of its sample (keys are unique, so the positions
// are a permutation: no sort, no scatter hazard).  Exact whatever total is; only ranks < cap are written.
__global__ void __launch_bounds__(256) k_rank_place(const float *pred, int hw, int cap, const unsigned long long *keys, const int32_t *total, float *boxes,
                                                    float *scores)
{
    __shared__ unsigned long long tile[EV_TILE];
    const int b = blockIdx.y;
    const int n = min(total[b], 2 * hw);
    if ((int)(blockIdx.x * 256) >= n) return;                    // the whole workgroup leaves together
    const unsigned long long *kb = keys + (size_t)b * 2 * hw;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long mine = i < n ? kb[i] : ~0ull;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += EV_TILE) {
        __syncthreads();
        for (int q = threadIdx.x; q < EV_TILE; q += 256) tile[q] = j0 + q < n ? kb[j0 + q] : 0ull;   // 0 is below every key
        __syncthreads();
#pragma unroll 8
        for (int q = 0; q < EV_TILE; ++q) rank += tile[q] > mine ? 1 : 0;
    }
    if (i >= n || rank >= cap) return;
    const unsigned idx = 0xFFFFFFFFu - (unsigned)(mine & 0xFFFFFFFFull);
    if (idx >= (unsigned)(2 * hw)) return;
    const int a = idx >= (unsigned)hw ? 1 : 0, px = (int)idx - a * hw;
    const float *p = pred + (size_t)b * 32 * hw;
    float *ob = boxes + ((size_t)b * cap + rank) * 7;
    for (int k = 0; k < 7; ++k) ob[k] = p[(size_t)(18 + 7 * a + k) * hw + px];
    scores[(size_t)b * cap + rank] = p[(size_t)(2 * a + 1) * hw + px];
}

// iou[i][r] = bird's-eye IoU of candidate i (a survivor of the suppression) with labelled row r; NaN where there is no pair
__global__ void __launch_bounds__(256) k_rank_iou(const float *boxes, const int32_t *keep, const int *count, int n_max, const float *refs, int R, double *iou)
{
    const int n = min(*count, n_max);
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(t / R), r = (int)(t - (long long)i * R);
    if (i >= n) return;
    double v = __longlong_as_double(0x7ff8000000000000ll);
    const float *rb = refs + (size_t)r * 9;
    if (keep[i] != 0 && rb[8] == 1.0f) {
        double r1[4][2], r2[4][2];
        ev_rect(boxes + (size_t)i * 7, r1);
        ev_rect(rb, r2);
        v = ev_bev_iou(r1, r2);
    }
    iou[(size_t)i * R + r] = v;
}

// One wave per IoU threshold walks the survivors in rank order: the best row not yet taken at this threshold (lanes stride over
// the rows; IoU ties go to the lower row), a pair iff its IoU > t.  The waves meet in an LDS bit mask, written out at the end.
__global__ void __launch_bounds__(1024) k_rank_match(const double *iou, const int32_t *keep, const int *count, int n_max, int R, const double *thr, int nthr,
                                                     unsigned *tpmask)
{
    __shared__ unsigned msk[EV_CAP];
    const int n = min(min(*count, n_max), EV_CAP);
    for (int q = threadIdx.x; q < n; q += blockDim.x) msk[q] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < nthr) {
        const double t = thr[wave];
        unsigned long long taken = 0ull;                         // bit k: row lane + 64 k is taken
        for (int i = 0; i < n; ++i) {
            if (keep[i] == 0) continue;
            double best = -__longlong_as_double(0x7ff0000000000000ll);
            int bestr = 0x7fffffff;
            for (int r = lane, k = 0; r < R; r += 64, ++k) {
                if ((taken >> k) & 1ull) continue;
                const double v = iou[(size_t)i * R + r];
                if (v > best) { best = v; bestr = r; }           // NaN never wins; ascending r keeps the lower row on a tie
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const int orow = __shfl_xor(bestr, o, 64);
                if (ob > best || (ob == best && orow < bestr)) { best = ob; bestr = orow; }
            }
            if (best > t && bestr < R) {
                if ((bestr & 63) == lane) taken |= 1ull << (bestr >> 6);
                if (lane == 0) atomicOr(&msk[i], 1u << wave);
            }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < n; q += blockDim.x) tpmask[q] = msk[q];
}

// Order-preserving append of one sample's survivors (score, tpmask) at the cursor; state = {cursor, n_gt, truncated samples, -}.
// The cursor keeps counting past the capacity (the summary raises then); nothing past it is written.
__global__ void __launch_bounds__(1024) k_rank_accumulate(const float *scores, const unsigned *tpmask, const int32_t *keep, const int *count, const int *total,
                                                          int n_max, const float *refs, int R, float *acc_scores, unsigned *acc_tp, long long capacity,
                                                          long long *state)
{
    __shared__ int wsum[16];
    __shared__ long long base_s;
    __shared__ int ngt_s;
    const int n = min(*count, n_max);
    if (threadIdx.x == 0) { base_s = state[0]; ngt_s = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int i = c0 + threadIdx.x;
        const bool ok = i < n && keep[i] != 0;
        const unsigned long long bal = __ballot(ok);
        const int before = __popcll(bal & ((1ull << lane) - 1));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        long long pos = base_s + before;
        for (int w = 0; w < wave; ++w) pos += wsum[w];
        if (ok && pos >= 0 && pos < capacity) { acc_scores[pos] = scores[i]; acc_tp[pos] = tpmask[i]; }
        __syncthreads();
        if (threadIdx.x == 0) { int tot = 0; for (int w = 0; w < 16; ++w) tot += wsum[w]; base_s += tot; }
        __syncthreads();
    }
    for (int r0 = 0; r0 < R; r0 += 1024) {
        const int r = r0 + threadIdx.x;
        const unsigned long long bal = __ballot(r < R && refs[(size_t)r * 9 + 8] == 1.0f);
        if (lane == 0) atomicAdd(&ngt_s, (int)__popcll(bal));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        state[0] = base_s;
        state[1] += ngt_s;
        if (*total > n_max) state[2] += 1;
    }
}

// Global rank of every accumulated detection by counting over (orderable score, ~index) keys; its tpmask goes to that rank
__global__ void __launch_bounds__(256) k_ap_rank(const float *acc_scores, const unsigned *acc_tp, const long long *state, long long capacity, unsigned *sorted_tp)
{
    __shared__ unsigned long long tile[EV_TILE];
    const int n = (int)max(0ll, min(state[0], capacity));
    if ((int)(blockIdx.x * 256) >= n) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long mine = i < n ? ev_key(acc_scores[i], (unsigned)i) : ~0ull;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += EV_TILE) {
        __syncthreads();
        for (int q = threadIdx.x; q < EV_TILE; q += 256) tile[q] = j0 + q < n ? ev_key(acc_scores[j0 + q], (unsigned)(j0 + q)) : 0ull;
        __syncthreads();
#pragma unroll 8
        for (int q = 0; q < EV_TILE; ++q) rank += tile[q] > mine ? 1 : 0;
    }
    if (i < n && rank < n) sorted_tp[rank] = acc_tp[i];
}

// One workgroup per threshold: c_k by a chunked inclusive scan with carry, p_k = c_k / k, the maximum of p_k per highest recall
// level reached (integer max on the bit pattern of a non-negative double: order-independent), then the 40-term sum.
__global__ void __launch_bounds__(1024) k_ap_curve(const unsigned *sorted_tp, const long long *state, long long capacity, double *out_ap, long long *out_counts)
{
    __shared__ unsigned long long M[EV_LEVELS + 1];
    __shared__ int wsum[16];
    __shared__ long long carry_s;
    const int t = blockIdx.x;
    const int n = (int)max(0ll, min(state[0], capacity));
    const long long n_gt = state[1];
    if (threadIdx.x <= EV_LEVELS) M[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int k = c0 + threadIdx.x;
        const bool bit = k < n && ((sorted_tp[k] >> t) & 1u);
        const unsigned long long bal = __ballot(bit);
        const int incl = __popcll(bal & ((2ull << lane) - 1));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        long long c = carry_s + incl;
        for (int w = 0; w < wave; ++w) c += wsum[w];
        if (k < n && n_gt > 0) {
            const double p = (double)c / (double)(k + 1);
            const long long j = min((long long)EV_LEVELS, 40 * c / n_gt);
            atomicMax(&M[j], (unsigned long long)__double_as_longlong(p));
        }
        __syncthreads();
        if (threadIdx.x == 0) { int tot = 0; for (int w = 0; w < 16; ++w) tot += wsum[w]; carry_s += tot; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double ap = __longlong_as_double(0x7ff8000000000000ll);
        if (n_gt > 0) {
            double sum = 0.0;
            for (int j = 1; j <= EV_LEVELS; ++j) {
                unsigned long long m = 0ull;
                for (int q = j; q <= EV_LEVELS; ++q) m = max(m, M[q]);
                sum += __longlong_as_double((long long)m);
            }
            ap = sum / 40.0;
        }
        out_ap[t] = ap;
        out_counts[t] = carry_s;
    }
}

}  // namespace

extern "C" int dcf_eval_score_filter(const float *pred, int B, int h, int w, float thr, int cap, float *boxes, int32_t *count, dcf_stream_t stream)
{
    DCF_REQUIRE(pred && boxes && count && B > 0 && h > 0 && w > 0 && cap > 0, "dcf_eval_score_filter: bad arguments");
    hipStream_t s = S(stream);
    DCF_LAUNCH_B("eval_score_filter", (double)B * h * w * 2 * 4.0, s, hipLaunchKernelGGL(k_eval_score_filter, dim3(B), dim3(1024), 0, s, pred, h * w, thr, cap, boxes, count));
    return DCF_OK;
}

extern "C" size_t dcf_eval_nms_workspace_bytes(int n_max)
{
    const size_t words = (size_t)(n_max + 63) / 64;
    return sizeof(EvGeom) * (size_t)n_max + 8 * words * (size_t)n_max + 64;
}

extern "C" int dcf_eval_nms(const float *boxes, const int32_t *count_dev, int n_max, int mode, double iou_threshold, int32_t *keep, int32_t *nkeep,
                            void *ws, dcf_stream_t stream)
{
    DCF_REQUIRE(boxes && keep && nkeep && ws && n_max >= 0 && n_max <= EV_CAP, "dcf_eval_nms: at most %d boxes per call (got %d)", EV_CAP, n_max);
    DCF_REQUIRE(mode == 0 || mode == 1 || mode == 2, "dcf_eval_nms: mode 0 = separating axes, 1 = 3-D IoU, 2 = bird's-eye IoU");
    hipStream_t s = S(stream);
    if (n_max == 0) { DCF_HIP(hipMemsetAsync(nkeep, 0, sizeof(int32_t), s)); return DCF_OK; }
    const int words = (n_max + 63) / 64;
    EvGeom *geom = (EvGeom *)ws;
    unsigned long long *mask = (unsigned long long *)((char *)ws + ((sizeof(EvGeom) * (size_t)n_max + 63) & ~(size_t)63));
    DCF_LAUNCH("eval_prep", s, hipLaunchKernelGGL(k_eval_prep, dim3(cdiv(n_max, 256)), dim3(256), 0, s, boxes, count_dev, n_max, geom));
    DCF_LAUNCH("eval_pairs", s, hipLaunchKernelGGL(k_eval_pairs, dim3(cdiv((int64_t)n_max * words, 256)), dim3(256), 0, s, geom, count_dev, n_max, mode, iou_threshold, words, mask));
    DCF_LAUNCH("eval_scan", s, hipLaunchKernelGGL(k_eval_scan, dim3(1), dim3(64), 0, s, mask, count_dev, n_max, words, keep, nkeep));
    return DCF_OK;
}

extern "C" int dcf_eval_match(const float *pred_boxes, int npred, const float *ref_boxes, int nref_rows, const double *thresholds_dev, int nthr,
                              int32_t *tp_counters, dcf_stream_t stream)
{
    DCF_REQUIRE(ref_boxes && thresholds_dev && tp_counters && nthr >= 1 && nthr <= 32 && npred >= 0 && nref_rows >= 0, "dcf_eval_match: bad arguments");
    if (npred == 0) return DCF_OK;
    DCF_REQUIRE(pred_boxes, "dcf_eval_match: null predictions");
    hipStream_t s = S(stream);
    DCF_LAUNCH("eval_match", s, hipLaunchKernelGGL(k_eval_match, dim3(cdiv(npred, 256)), dim3(256), 0, s, pred_boxes, npred, ref_boxes, nref_rows, thresholds_dev, nthr, tp_counters));
    return DCF_OK;
}

// ------------------------------------------------------------------ ranked evaluation: entries
extern "C" size_t dcf_eval_rank_workspace_bytes(int B, int h, int w)
{
    return 8 * (size_t)B * 2 * (size_t)h * (size_t)w + 64;
}

extern "C" int dcf_eval_rank_filter(const float *pred, int B, int h, int w, float thr, int cap, float *boxes, float *scores, int32_t *count, int32_t *total,
                                    void *ws, dcf_stream_t stream)
{
    DCF_REQUIRE(pred && boxes && scores && count && total && ws && B > 0 && B <= 65535 && h > 0 && w > 0 && cap > 0 && (int64_t)h * w <= (1 << 29),
                "dcf_eval_rank_filter: bad arguments");
    hipStream_t s = S(stream);
    const int hw = h * w;
    unsigned long long *keys = (unsigned long long *)ws;
    DCF_LAUNCH_B("eval_rank_compact", (double)B * hw * 2 * 4.0, s, hipLaunchKernelGGL(k_rank_compact, dim3(B), dim3(1024), 0, s, pred, hw, thr, cap, keys, count, total));
    DCF_LAUNCH("eval_rank_place", s, hipLaunchKernelGGL(k_rank_place, dim3(cdiv(2 * (int64_t)hw, 256), B), dim3(256), 0, s, pred, hw, cap, keys, total, boxes, scores));
    return DCF_OK;
}

extern "C" size_t dcf_eval_match_ranked_workspace_bytes(int n_max, int R)
{
    return 8 * (size_t)(n_max > 0 ? n_max : 0) * (size_t)(R > 0 ? R : 0) + 64;
}

extern "C" int dcf_eval_match_ranked(const float *boxes, const int32_t *keep, const int32_t *count_dev, int n_max, const float *refs, int R,
                                     const double *thresholds_dev, int nthr, uint32_t *tpmask, void *ws, dcf_stream_t stream)
{
    DCF_REQUIRE(boxes && keep && count_dev && thresholds_dev && tpmask && ws && n_max > 0 && n_max <= EV_CAP && R >= 0 && R <= 4096 && nthr >= 1 && nthr <= 16,
                "dcf_eval_match_ranked: at most %d boxes, 4096 label rows and 16 thresholds per call (got %d, %d, %d)", EV_CAP, n_max, R, nthr);
    DCF_REQUIRE(R == 0 || refs, "dcf_eval_match_ranked: null label rows");
    hipStream_t s = S(stream);
    double *iou = (double *)ws;
    if (R > 0)
        DCF_LAUNCH("eval_rank_iou", s, hipLaunchKernelGGL(k_rank_iou, dim3(cdiv((int64_t)n_max * R, 256)), dim3(256), 0, s, boxes, keep, count_dev, n_max, refs, R, iou));
    DCF_LAUNCH("eval_rank_match", s, hipLaunchKernelGGL(k_rank_match, dim3(1), dim3(64 * nthr), 0, s, iou, keep, count_dev, n_max, R, thresholds_dev, nthr, tpmask));
    return DCF_OK;
}

extern "C" int dcf_eval_accumulate(const float *scores, const uint32_t *tpmask, const int32_t *keep, const int32_t *count_dev, const int32_t *total_dev, int n_max,
                                   const float *refs, int R, float *acc_scores, uint32_t *acc_tpmask, int64_t capacity, int64_t *state, dcf_stream_t stream)
{
    DCF_REQUIRE(scores && tpmask && keep && count_dev && total_dev && acc_scores && acc_tpmask && state && n_max > 0 && n_max <= EV_CAP && R >= 0 &&
                capacity > 0 && capacity <= (1 << 30), "dcf_eval_accumulate: bad arguments");
    DCF_REQUIRE(R == 0 || refs, "dcf_eval_accumulate: null label rows");
    hipStream_t s = S(stream);
    DCF_LAUNCH("eval_accumulate", s, hipLaunchKernelGGL(k_rank_accumulate, dim3(1), dim3(1024), 0, s, scores, tpmask, keep, count_dev, total_dev, n_max, refs, R,
                                                        acc_scores, acc_tpmask, (long long)capacity, (long long *)state));
    return DCF_OK;
}

extern "C" size_t dcf_eval_ap_workspace_bytes(int64_t capacity)
{
    return 4 * (size_t)(capacity > 0 ? capacity : 0) + 64;
}

extern "C" int dcf_eval_ap(const float *acc_scores, const uint32_t *acc_tpmask, const int64_t *state, int64_t capacity, int nthr, double *out_ap,
                           int64_t *out_counts, void *ws, dcf_stream_t stream)
{
    DCF_REQUIRE(acc_scores && acc_tpmask && state && out_ap && out_counts && ws && capacity > 0 && capacity <= (1 << 30) && nthr >= 1 && nthr <= 32,
                "dcf_eval_ap: bad arguments");
    hipStream_t s = S(stream);
    unsigned *sorted_tp = (unsigned *)ws;
    DCF_LAUNCH("eval_ap_rank", s, hipLaunchKernelGGL(k_ap_rank, dim3(cdiv(capacity, 256)), dim3(256), 0, s, acc_scores, acc_tpmask, (const long long *)state,
                                                     (long long)capacity, sorted_tp));
    DCF_LAUNCH("eval_ap_curve", s, hipLaunchKernelGGL(k_ap_curve, dim3(nthr), dim3(1024), 0, s, sorted_tp, (const long long *)state, (long long)capacity, out_ap,
                                                      (long long *)out_counts));
    return DCF_OK;
}

// ------------------------------------------------------------------ KITTI-style protocol (eval_protocol: kitti)
// The third outcome (ignored), the difficulty dimension and the z axis on top of the ranked evaluation above; evalkitti.py is the
// host statement.  Mask words carry bit 10 d + t for difficulty d (easy, moderate, hard) and threshold t, one word per metric
// (bird's-eye, 3-D).  The kernels above are not touched.
namespace {

constexpr int EV_BITS = 10;              // bits per difficulty in a mask word

struct EvFlagParam {                     // by value: nothing has to reach the device first
    float C[12];                         // the frame's [4][3] projection matrix, row-major: [x, y, z, 1] . C = (u d, v d, d)
    double H, W;                         // image size the 2-D box is clamped to
    double min_height[3];
    double overlap;
};

// flags[i]: bit d iff the projected height of candidate i is below min_height[d]; bit 3 iff more than `overlap` of its 2-D box lies
// in one DontCare rectangle (evalkitti.det_flags).  fp64 on the fp32 entries, in the stated order (no contraction).
__global__ void __launch_bounds__(256) k_kitti_flags(const float *boxes, const int *count, int n_max, EvFlagParam p, const float *dontcare, int D, unsigned *flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = min(*count, n_max);
    if (i >= n) return;
    const float *b = boxes + (size_t)i * 7;
    double rect[4][2];
    ev_rect(b, rect);
    const double z = b[2], h = b[5];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double umin = inf, vmin = inf, umax = -inf, vmax = -inf;
    int front = 0;
    for (int s = 0; s < 2; ++s) {
        const double zz = s == 0 ? z - h / 2 : z + h / 2;
        for (int k = 0; k < 4; ++k) {
            const double x = rect[k][0], y = rect[k][1];
            const double d = ((x * (double)p.C[2] + y * (double)p.C[5]) + zz * (double)p.C[8]) + (double)p.C[11];
            if (!(d > 0)) continue;
            ++front;
            const double ud = ((x * (double)p.C[0] + y * (double)p.C[3]) + zz * (double)p.C[6]) + (double)p.C[9];
            const double vd = ((x * (double)p.C[1] + y * (double)p.C[4]) + zz * (double)p.C[7]) + (double)p.C[10];
            const double u = fmin(fmax(ud / d, 0.0), p.W), v = fmin(fmax(vd / d, 0.0), p.H);
            umin = fmin(umin, u); umax = fmax(umax, u);
            vmin = fmin(vmin, v); vmax = fmax(vmax, v);
        }
    }
    double height = 0.0, area = 0.0;
    if (front > 0) { height = vmax - vmin; area = (umax - umin) * height; }
    unsigned f = 0;
    for (int d = 0; d < 3; ++d)
        if (height < p.min_height[d]) f |= 1u << d;
    if (area > 0) {
        for (int q = 0; q < D; ++q) {
            const float *rc = dontcare + (size_t)q * 4;
            const double iw = fmin(umax, (double)rc[2]) - fmax(umin, (double)rc[0]);
            const double ih = fmin(vmax, (double)rc[3]) - fmax(vmin, (double)rc[1]);
            if (iw > 0 && ih > 0 && iw * ih / area > p.overlap) { f |= 8u; break; }
        }
    }
    flags[i] = f;
}

// iou_bev[i][r], iou_3d[i][r] of candidate i (a survivor) with labelled row r, both from one clip; NaN where there is no pair
__global__ void __launch_bounds__(256) k_kitti_iou(const float *boxes, const int32_t *keep, const int *count, int n_max, const float *refs, int R, double *iou_bev,
                                                   double *iou_3d)
{
    const int n = min(*count, n_max);
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(t / R), r = (int)(t - (long long)i * R);
    if (i >= n) return;
    double vb = __longlong_as_double(0x7ff8000000000000ll), v3 = vb;
    const float *pb = boxes + (size_t)i * 7, *rb = refs + (size_t)r * 9;
    if (keep[i] != 0 && rb[8] == 1.0f) {
        double r1[4][2], r2[4][2], poly[12][2];
        ev_rect(pb, r1);
        ev_rect(rb, r2);
        const int nv = ev_clip(r1, r2, poly);
        const double ia = nv >= 3 ? ev_shoelace(poly, nv) : 0.0;
        const double a1 = ev_shoelace(r1, 4), a2 = ev_shoelace(r2, 4);
        vb = ia / (a1 + a2 - ia);
        const double z1 = pb[2], h1 = pb[5], z2 = rb[2], h2 = rb[5];
        const double zov = fmax(0.0, fmin(z1 + h1 / 2, z2 + h2 / 2) - fmax(z1 - h1 / 2, z2 - h2 / 2));
        const double iv = ia * zov;
        v3 = iv / (a1 * h1 + a2 * h2 - iv);
    }
    iou_bev[(size_t)i * R + r] = vb;
    iou_3d[(size_t)i * R + r] = v3;
}

// One workgroup per (metric, difficulty), k_rank_match's shape inside: one wave per threshold walks the survivors in rank order.
// (A) the best counted row not yet taken, a true positive iff its IoU > t; else (B) ignored iff an ignored row has IoU > t; else (C)
// ignored iff flag bit d or 3 is set.  Each workgroup owns one 10-bit field of the output words (zeroed by the entry): an integer OR.
__global__ void __launch_bounds__(1024) k_kitti_match(const double *iou_bev, const double *iou_3d, const int32_t *keep, const int *count, int n_max, const float *refs,
                                                      const int32_t *levels, int R, const unsigned *flags, const double *thr, int nthr, unsigned *tpmask,
                                                      unsigned *igmask)
{
    __shared__ unsigned tp_s[EV_CAP], ig_s[EV_CAP];
    const int m = blockIdx.x / 3, d = blockIdx.x - 3 * m;
    const double *iou = m == 0 ? iou_bev : iou_3d;
    const int n = min(min(*count, n_max), EV_CAP);
    for (int q = threadIdx.x; q < n; q += blockDim.x) { tp_s[q] = 0u; ig_s[q] = 0u; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < nthr) {
        const double t = thr[wave];
        unsigned long long counted = 0ull, ignored = 0ull, taken = 0ull;      // bit k: row lane + 64 k
        for (int r = lane, k = 0; r < R; r += 64, ++k) {
            if (refs[(size_t)r * 9 + 8] != 1.0f) continue;
            const int lv = levels ? levels[r] : 0;
            if (lv <= d) counted |= 1ull << k; else ignored |= 1ull << k;
        }
        const unsigned fbits = (1u << d) | 8u;
        for (int i = 0; i < n; ++i) {
            if (keep[i] == 0) continue;
            double best = -__longlong_as_double(0x7ff0000000000000ll);
            int bestr = 0x7fffffff;
            const unsigned long long open = counted & ~taken;
            for (int r = lane, k = 0; r < R; r += 64, ++k) {
                if (!((open >> k) & 1ull)) continue;
                const double v = iou[(size_t)i * R + r];
                if (v > best) { best = v; bestr = r; }           // NaN never wins; ascending r keeps the lower row on a tie
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const int orow = __shfl_xor(bestr, o, 64);
                if (ob > best || (ob == best && orow < bestr)) { best = ob; bestr = orow; }
            }
            if (best > t && bestr < R) {                         // the same on every lane
                if ((bestr & 63) == lane) taken |= 1ull << (bestr >> 6);
                if (lane == 0) atomicOr(&tp_s[i], 1u << wave);
            } else {
                bool hit = false;
                for (int r = lane, k = 0; r < R; r += 64, ++k)
                    if (((ignored >> k) & 1ull) && iou[(size_t)i * R + r] > t) hit = true;
                const bool ig = __ballot(hit) != 0ull || (flags[i] & fbits) != 0u;
                if (ig && lane == 0) atomicOr(&ig_s[i], 1u << wave);
            }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < n; q += blockDim.x) {
        if (tp_s[q]) atomicOr(&tpmask[(size_t)m * n_max + q], tp_s[q] << (EV_BITS * d));
        if (ig_s[q]) atomicOr(&igmask[(size_t)m * n_max + q], ig_s[q] << (EV_BITS * d));
    }
}

// Order-preserving append of one sample's survivors (score, tpmask[2], igmask[2]) at the cursor; state = {cursor, n_gt[3], truncated
// samples, -, -, -}.  The cursor keeps counting past the capacity (the summary raises then); nothing past it is written.
__global__ void __launch_bounds__(1024) k_kitti_accumulate(const float *scores, const unsigned *tpmask, const unsigned *igmask, const int32_t *keep, const int *count,
                                                           const int *total, int n_max, const float *refs, const int32_t *levels, int R, float *acc_scores,
                                                           unsigned *acc_tp, unsigned *acc_ig, long long capacity, long long *state)
{
    __shared__ int wsum[16];
    __shared__ long long base_s;
    __shared__ int ngt_s[3];
    const int n = min(*count, n_max);
    if (threadIdx.x == 0) { base_s = state[0]; ngt_s[0] = 0; ngt_s[1] = 0; ngt_s[2] = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int i = c0 + threadIdx.x;
        const bool ok = i < n && keep[i] != 0;
        const unsigned long long bal = __ballot(ok);
        const int before = __popcll(bal & ((1ull << lane) - 1));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        long long pos = base_s + before;
        for (int w = 0; w < wave; ++w) pos += wsum[w];
        if (ok && pos >= 0 && pos < capacity) {
            acc_scores[pos] = scores[i];
            for (int m = 0; m < 2; ++m) {
                acc_tp[(size_t)m * capacity + pos] = tpmask[(size_t)m * n_max + i];
                acc_ig[(size_t)m * capacity + pos] = igmask[(size_t)m * n_max + i];
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) { int tot = 0; for (int w = 0; w < 16; ++w) tot += wsum[w]; base_s += tot; }
        __syncthreads();
    }
    for (int r0 = 0; r0 < R; r0 += 1024) {
        const int r = r0 + threadIdx.x;
        const bool valid = r < R && refs[(size_t)r * 9 + 8] == 1.0f;
        const int lv = valid && levels ? levels[r] : 0;
        for (int d = 0; d < 3; ++d) {
            const unsigned long long bal = __ballot(valid && lv <= d);
            if (lane == 0) atomicAdd(&ngt_s[d], (int)__popcll(bal));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        state[0] = base_s;
        for (int d = 0; d < 3; ++d) state[1 + d] += ngt_s[d];
        if (*total > n_max) state[4] += 1;
    }
}

// k_ap_rank for the four mask arrays: sorted [4][capacity] = tpmask[0], tpmask[1], igmask[0], igmask[1] in global rank order
__global__ void __launch_bounds__(256) k_kitti_ap_rank(const float *acc_scores, const unsigned *acc_tp, const unsigned *acc_ig, const long long *state,
                                                       long long capacity, unsigned *sorted)
{
    __shared__ unsigned long long tile[EV_TILE];
    const int n = (int)max(0ll, min(state[0], capacity));
    if ((int)(blockIdx.x * 256) >= n) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long mine = i < n ? ev_key(acc_scores[i], (unsigned)i) : ~0ull;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += EV_TILE) {
        __syncthreads();
        for (int q = threadIdx.x; q < EV_TILE; q += 256) tile[q] = j0 + q < n ? ev_key(acc_scores[j0 + q], (unsigned)(j0 + q)) : 0ull;
        __syncthreads();
#pragma unroll 8
        for (int q = 0; q < EV_TILE; ++q) rank += tile[q] > mine ? 1 : 0;
    }
    if (i < n && rank < n) {
        for (int m = 0; m < 2; ++m) {
            sorted[(size_t)m * capacity + rank] = acc_tp[(size_t)m * capacity + i];
            sorted[(size_t)(2 + m) * capacity + rank] = acc_ig[(size_t)m * capacity + i];
        }
    }
}

// One workgroup per (metric, difficulty, threshold): k_ap_curve with a second scan.  k counts the detections not ignored here, c the
// true positives among them; p = c / k enters the level reached by 40 c / n_gt[d] for the detections that stay.
__global__ void __launch_bounds__(1024) k_kitti_ap_curve(const unsigned *sorted, const long long *state, long long capacity, int nthr, double *out_ap,
                                                         long long *out_tp, long long *out_ig)
{
    __shared__ unsigned long long M[EV_LEVELS + 1];
    __shared__ int wsum_c[16], wsum_k[16];
    __shared__ long long carry_c, carry_k;
    const int blk = blockIdx.x, m = blk / (3 * nthr), d = (blk / nthr) % 3, t = blk % nthr;
    const int sh = EV_BITS * d + t;
    const unsigned *tp = sorted + (size_t)m * capacity, *ig = sorted + (size_t)(2 + m) * capacity;
    const int n = (int)max(0ll, min(state[0], capacity));
    const long long n_gt = state[1 + d];
    if (threadIdx.x <= EV_LEVELS) M[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) { carry_c = 0; carry_k = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int q = c0 + threadIdx.x;
        const bool stay = q < n && !((ig[q] >> sh) & 1u);
        const bool bit = stay && ((tp[q] >> sh) & 1u);
        const unsigned long long balc = __ballot(bit), balk = __ballot(stay);
        const unsigned long long upto = (2ull << lane) - 1;
        const int inclc = __popcll(balc & upto), inclk = __popcll(balk & upto);
        if (lane == 0) { wsum_c[wave] = __popcll(balc); wsum_k[wave] = __popcll(balk); }
        __syncthreads();
        long long c = carry_c + inclc, k = carry_k + inclk;
        for (int w = 0; w < wave; ++w) { c += wsum_c[w]; k += wsum_k[w]; }
        if (stay && n_gt > 0) {
            const double p = (double)c / (double)k;
            const long long j = min((long long)EV_LEVELS, 40 * c / n_gt);
            atomicMax(&M[j], (unsigned long long)__double_as_longlong(p));
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int totc = 0, totk = 0;
            for (int w = 0; w < 16; ++w) { totc += wsum_c[w]; totk += wsum_k[w]; }
            carry_c += totc; carry_k += totk;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double ap = __longlong_as_double(0x7ff8000000000000ll);
        if (n_gt > 0) {
            double sum = 0.0;
            for (int j = 1; j <= EV_LEVELS; ++j) {
                unsigned long long mx = 0ull;
                for (int q = j; q <= EV_LEVELS; ++q) mx = max(mx, M[q]);
                sum += __longlong_as_double((long long)mx);
            }
            ap = sum / 40.0;
        }
        out_ap[blk] = ap;
        out_tp[blk] = carry_c;
        out_ig[blk] = (long long)n - carry_k;
    }
}

}  // namespace

extern "C" int dcf_eval_det_flags(const float *boxes, const int32_t *count_dev, int n_max, const float *crt_host, const float *dontcare, int D, int image_h,
                                  int image_w, const double *min_height_host, double overlap, uint32_t *flags, dcf_stream_t stream)
{
    DCF_REQUIRE(boxes && count_dev && crt_host && min_height_host && flags && n_max > 0 && n_max <= EV_CAP && D >= 0 && D <= 4096 && image_h > 0 && image_w > 0,
                "dcf_eval_det_flags: at most %d boxes and 4096 DontCare rectangles per call (got %d, %d)", EV_CAP, n_max, D);
    DCF_REQUIRE(D == 0 || dontcare, "dcf_eval_det_flags: null DontCare rectangles");
    DCF_REQUIRE(overlap > 0.0 && overlap <= 1.0, "dcf_eval_det_flags: overlap must be in (0, 1]");
    EvFlagParam p;
    for (int k = 0; k < 12; ++k) p.C[k] = crt_host[k];
    for (int d = 0; d < 3; ++d) p.min_height[d] = min_height_host[d];
    p.H = (double)image_h; p.W = (double)image_w; p.overlap = overlap;
    hipStream_t s = S(stream);
    DCF_LAUNCH("eval_kitti_flags", s, hipLaunchKernelGGL(k_kitti_flags, dim3(cdiv(n_max, 256)), dim3(256), 0, s, boxes, count_dev, n_max, p, dontcare, D, flags));
    return DCF_OK;
}

extern "C" int dcf_eval_iou_levels(const float *boxes, const int32_t *keep, const int32_t *count_dev, int n_max, const float *refs, int R, double *iou_bev,
                                   double *iou_3d, dcf_stream_t stream)
{
    DCF_REQUIRE(boxes && keep && count_dev && n_max > 0 && n_max <= EV_CAP && R >= 0 && R <= 4096,
                "dcf_eval_iou_levels: at most %d boxes and 4096 label rows per call (got %d, %d)", EV_CAP, n_max, R);
    if (R == 0) return DCF_OK;
    DCF_REQUIRE(refs && iou_bev && iou_3d, "dcf_eval_iou_levels: null label rows or matrices");
    hipStream_t s = S(stream);
    DCF_LAUNCH("eval_kitti_iou", s, hipLaunchKernelGGL(k_kitti_iou, dim3(cdiv((int64_t)n_max * R, 256)), dim3(256), 0, s, boxes, keep, count_dev, n_max, refs, R, iou_bev, iou_3d));
    return DCF_OK;
}

extern "C" int dcf_eval_match_levels(const double *iou_bev, const double *iou_3d, const int32_t *keep, const int32_t *count_dev, int n_max, const float *refs,
                                     const int32_t *levels, int R, const uint32_t *flags, const double *thresholds_dev, int nthr, uint32_t *tpmask,
                                     uint32_t *igmask, dcf_stream_t stream)
{
    DCF_REQUIRE(keep && count_dev && flags && thresholds_dev && tpmask && igmask && n_max > 0 && n_max <= EV_CAP && R >= 0 && R <= 4096 && nthr >= 1 && nthr <= EV_BITS,
                "dcf_eval_match_levels: at most %d boxes, 4096 label rows and %d thresholds per call (got %d, %d, %d)", EV_CAP, EV_BITS, n_max, R, nthr);
    DCF_REQUIRE(R == 0 || (refs && iou_bev && iou_3d), "dcf_eval_match_levels: null label rows or matrices");
    hipStream_t s = S(stream);
    DCF_HIP(hipMemsetAsync(tpmask, 0, sizeof(uint32_t) * 2 * (size_t)n_max, s));
    DCF_HIP(hipMemsetAsync(igmask, 0, sizeof(uint32_t) * 2 * (size_t)n_max, s));
    DCF_LAUNCH("eval_kitti_match", s, hipLaunchKernelGGL(k_kitti_match, dim3(6), dim3(64 * nthr), 0, s, iou_bev, iou_3d, keep, count_dev, n_max, refs, levels, R, flags,
                                                         thresholds_dev, nthr, tpmask, igmask));
    return DCF_OK;
}

extern "C" int dcf_eval_accumulate_levels(const float *scores, const uint32_t *tpmask, const uint32_t *igmask, const int32_t *keep, const int32_t *count_dev,
                                          const int32_t *total_dev, int n_max, const float *refs, const int32_t *levels, int R, float *acc_scores,
                                          uint32_t *acc_tpmask, uint32_t *acc_igmask, int64_t capacity, int64_t *state, dcf_stream_t stream)
{
    DCF_REQUIRE(scores && tpmask && igmask && keep && count_dev && total_dev && acc_scores && acc_tpmask && acc_igmask && state && n_max > 0 && n_max <= EV_CAP &&
                R >= 0 && capacity > 0 && capacity <= (1 << 30), "dcf_eval_accumulate_levels: bad arguments");
    DCF_REQUIRE(R == 0 || refs, "dcf_eval_accumulate_levels: null label rows");
    hipStream_t s = S(stream);
    DCF_LAUNCH("eval_kitti_accumulate", s, hipLaunchKernelGGL(k_kitti_accumulate, dim3(1), dim3(1024), 0, s, scores, tpmask, igmask, keep, count_dev, total_dev, n_max, refs,
                                                              levels, R, acc_scores, acc_tpmask, acc_igmask, (long long)capacity, (long long *)state));
    return DCF_OK;
}

extern "C" size_t dcf_eval_ap_levels_workspace_bytes(int64_t capacity)
{
    return 16 * (size_t)(capacity > 0 ? capacity : 0) + 64;
}

extern "C" int dcf_eval_ap_levels(const float *acc_scores, const uint32_t *acc_tpmask, const uint32_t *acc_igmask, const int64_t *state, int64_t capacity, int nthr,
                                  double *out_ap, int64_t *out_tp, int64_t *out_ignored, void *ws, dcf_stream_t stream)
{
    DCF_REQUIRE(acc_scores && acc_tpmask && acc_igmask && state && out_ap && out_tp && out_ignored && ws && capacity > 0 && capacity <= (1 << 30) && nthr >= 1 &&
                nthr <= EV_BITS, "dcf_eval_ap_levels: bad arguments");
    hipStream_t s = S(stream);
    unsigned *sorted = (unsigned *)ws;
    DCF_LAUNCH("eval_kitti_ap_rank", s, hipLaunchKernelGGL(k_kitti_ap_rank, dim3(cdiv(capacity, 256)), dim3(256), 0, s, acc_scores, acc_tpmask, acc_igmask,
                                                           (const long long *)state, (long long)capacity, sorted));
    DCF_LAUNCH("eval_kitti_ap_curve", s, hipLaunchKernelGGL(k_kitti_ap_curve, dim3(6 * nthr), dim3(1024), 0, s, sorted, (const long long *)state, (long long)capacity, nthr,
                                                            out_ap, (long long *)out_tp, (long long *)out_ignored));
    return DCF_OK;
}
