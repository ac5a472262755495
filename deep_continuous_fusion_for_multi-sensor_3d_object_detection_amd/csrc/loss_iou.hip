// loss_iou.hip -- the rotated-IoU regression term of `loss_sampling: anchor` (`iou_loss_gain`): for every positive
// anchor the IoU of the head's decoded box p with its label q and the derivative by the anchor's seven offsets, in fp64 on the fp32 inputs.
// loss.anchor_iou_terms / loss.iou_value_grad are the host statements; tests/test_gpu_loss_iou.py pins the kernels to them.
//
// Shape: positives are a few hundred among the 2 HW anchors, and a lane's work is a long serial fp64 chain, so a thread per cell would
// make every wave wait for its one busy lane (section 20's finding).  A workgroup scans IL_CHUNK anchors, compacts the positive ones in
// index order into LDS (ballot + wave counts: no atomics), then gives each positive a lane of its own; most workgroups find none and end
// after the scan.  The per-pair geometry keeps no polygon: each of p's four edges is clipped parametrically against q's four half-planes
// and each of q's against p's; the pieces are the boundary of the intersection, so the area is half the sum of their cross products, and
// the pieces of p's edges (length, midpoint) are the derivative.  All loops have constant bounds and are unrolled: no scratch.
#include "dcf_common.h"

namespace {

constexpr int IL_THREADS = 256;
constexpr int IL_WAVES = IL_THREADS / 64;
constexpr int IL_CHUNK = 2048;                 // anchors per workgroup (8 scan passes)

__host__ __device__ __forceinline__ float il_sample_weight(int reduction, int B) { return reduction == 2 ? 1.f / (float)B : 1.f; }

struct IouArgs {
    const float *reg, *anc, *boxes;
    const int32_t *target, *counts;
    int64_t reg_bs, greg_bs;
    float *greg;
    double *ws, *iou_map;
    int max_box, box_stride, b0, B, HW, kind, reduction, G;
    float gain;
};

// evalgeom.bev_rect with the centre, cos and sin given: counter-clockwise, corner k = (sl, sw)[k] half-sizes along / across the heading
__device__ __forceinline__ void il_rect(double cx, double cy, double l, double w, double c, double s, double (&X)[4], double (&Y)[4])
{
    const double hl = l / 2, hw = w / 2;
    const double sl[4] = {-1, 1, 1, -1}, sw[4] = {-1, -1, 1, 1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        X[k] = cx + sl[k] * hl * c - sw[k] * hw * s;
        Y[k] = cy + sl[k] * hl * s + sw[k] * hw * c;
    }
}

// The edge A -> B against the four half-planes of the rectangle R: the piece inside is A + t (B - A), t in [t0, t1]; empty when t1 <= t0.
// Strictly left of an edge of R is inside; side values and crossing parameter are ev_clip's.  CLOSED: an edge ON a line of R (both side
// values exactly 0) stays, so that of two coincident edges one is kept and one dropped.  NaN compares false everywhere: empty.
template <bool CLOSED>
__device__ __forceinline__ void il_edge(double ax, double ay, double bx, double by, const double (&RX)[4], const double (&RY)[4], double &t0,
                                        double &t1)
{
    t0 = 0.0; t1 = 1.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int j1 = (j + 1) & 3;
        const double ex = RX[j1] - RX[j], ey = RY[j1] - RY[j];
        const double sa = ex * (ay - RY[j]) - ey * (ax - RX[j]);
        const double sb = ex * (by - RY[j]) - ey * (bx - RX[j]);
        const bool ina = sa > 0, inb = sb > 0;
        if (ina != inb) {
            const double t = sa / (sa - sb);             // opposite sides: never 0/0, always in [0, 1]
            if (ina) t1 = fmin(t1, t); else t0 = fmax(t0, t);
        } else if (!ina && !(CLOSED && sa == 0 && sb == 0)) {
            t1 = -1.0;
        }
    }
}

__device__ __forceinline__ bool il_finite7(const double (&v)[7])
{
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 7; ++c) ok = ok && isfinite(v[c]);
    return ok;
}

// loss.iou_value_grad for one pair: p, q = (x, y, z, l, w, h, yaw), kind 0 = 3-D, 1 = bird's-eye; returns the IoU, g = d IoU / d p
__device__ double il_pair(const double (&p)[7], const double (&q)[7], int kind, double (&g)[7])
{
    const double x = p[0] - q[0], y = p[1] - q[1], l = p[3], w = p[4], h = p[5];
    const double c = cos(p[6]), s = sin(p[6]);
    double PX[4], PY[4], QX[4], QY[4];
    il_rect(x, y, l, w, c, s, PX, PY);
    il_rect(0.0, 0.0, q[3], q[4], cos(q[6]), sin(q[6]), QX, QY);
    const double nx[4] = {s, c, -s, -c}, ny[4] = {-c, s, c, -s};
    double twice = 0.0, len[4], dIx = 0.0, dIy = 0.0, dIyaw = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3;
        double t0, t1;
        il_edge<true>(PX[k], PY[k], PX[k1], PY[k1], QX, QY, t0, t1);
        const double d = fmax(0.0, t1 - t0), tm = 0.5 * (t0 + t1);
        twice += d * (PX[k] * PY[k1] - PY[k] * PX[k1]);
        len[k] = d * ((k & 1) ? w : l);
        const double mx = PX[k] + tm * (PX[k1] - PX[k]), my = PY[k] + tm * (PY[k1] - PY[k]);
        dIx += nx[k] * len[k];
        dIy += ny[k] * len[k];
        dIyaw += len[k] * (ny[k] * (mx - x) - nx[k] * (my - y));
    }
    double twice_q = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3;
        double t0, t1;
        il_edge<false>(QX[k], QY[k], QX[k1], QY[k1], PX, PY, t0, t1);
        twice_q += fmax(0.0, t1 - t0) * (QX[k] * QY[k1] - QY[k] * QX[k1]);
    }
    const double I = 0.5 * (twice + twice_q);
    const double dIl = 0.5 * (len[1] + len[3]), dIw = 0.5 * (len[0] + len[2]);
    double zo = 1.0, dzz = 0.0, dzh = 0.0, size, vq, dSl, dSw, dSh;
    if (kind == 1) {
        size = l * w; vq = q[3] * q[4];
        dSl = w; dSw = l; dSh = 0.0;
    } else {
        const double top_p = p[2] + h / 2, bot_p = p[2] - h / 2, top_q = q[2] + q[5] / 2, bot_q = q[2] - q[5] / 2;
        zo = fmax(0.0, fmin(top_p, top_q) - fmax(bot_p, bot_q));
        const double lower_top = (top_p < top_q && zo > 0) ? 1.0 : 0.0, higher_bot = (bot_p > bot_q && zo > 0) ? 1.0 : 0.0;
        dzz = lower_top - higher_bot; dzh = 0.5 * (lower_top + higher_bot);
        size = l * w * h; vq = q[3] * q[4] * q[5];
        dSl = w * h; dSw = l * h; dSh = l * w;
    }
    const double I3 = I * zo, U = size + vq - I3;
    const double dI3[7] = {dIx * zo, dIy * zo, I * dzz, dIl * zo, dIw * zo, I * dzh, dIyaw * zo};
    const double dS[7] = {0.0, 0.0, 0.0, dSl, dSw, dSh, 0.0};
    const bool ok = il_finite7(p) && il_finite7(q);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
    for (int k = 0; k < 7; ++k) g[k] = ok ? (dI3[k] * U - I3 * (dS[k] - dI3[k])) / (U * U) : nan;
    return ok ? I3 / U : nan;
}

// grid (G, B - b0): workgroup g of sample b takes the anchors [g IL_CHUNK, (g + 1) IL_CHUNK) of the sample's 2 HW.  ws slot (b, g) =
// (sum of 1 - IoU, sum of IoU) over its positives in index order.  greg: each positive's seven elements get the term's gradient ADDED
// by the one lane that owns the positive; nothing else is written.  iou_map (optional): IoU for a positive anchor, 0 otherwise.
__global__ void __launch_bounds__(IL_THREADS) k_loss_anchor_iou(IouArgs a)
{
    __shared__ int s_list[IL_CHUNK];
    __shared__ double s_iou[IL_CHUNK];
    __shared__ int s_wcnt[IL_WAVES];
    const int g = blockIdx.x, b = a.b0 + blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int HW = a.HW;
    const int64_t n2 = 2 * (int64_t)HW, lo = (int64_t)g * IL_CHUNK;
    const int32_t *tg = a.target + (int64_t)b * n2;
    double *map = a.iou_map ? a.iou_map + (int64_t)b * n2 : nullptr;
    int cnt = 0;
    for (int pass = 0; pass < IL_CHUNK / IL_THREADS; ++pass) {
        const int off = pass * IL_THREADS + tid;
        const int64_t j = lo + off;
        bool pos = false;
        if (j < n2) {
            const int t = tg[j];
            pos = t >= 0 && t < a.max_box;
            if (map && !pos) map[j] = 0.0;
        }
        const unsigned long long bal = __ballot(pos);
        if (lane == 0) s_wcnt[wv] = __popcll(bal);
        __syncthreads();
        int base = cnt, tot = 0;
#pragma unroll
        for (int v = 0; v < IL_WAVES; ++v) {
            const int c = s_wcnt[v];
            base += v < wv ? c : 0;
            tot += c;
        }
        if (pos) s_list[base + __popcll(bal & ((1ull << lane) - 1ull))] = off;
        cnt += tot;
        __syncthreads();
    }
    const double npos = (double)max(a.counts[4 * b], 1);
    const double gscale = -((double)il_sample_weight(a.reduction, a.B) * (double)a.gain) / npos;
    const float *r = a.reg + b * a.reg_bs;
    float *gr = a.greg + b * a.greg_bs;
    const float *bx = a.boxes + (int64_t)b * a.max_box * a.box_stride;
    for (int i = tid; i < cnt; i += IL_THREADS) {
        const int64_t j = lo + s_list[i];
        const int an = j >= HW ? 1 : 0;
        const int cell = (int)(j - (int64_t)an * HW);
        const int k = tg[j];                               // in [0, max_box): checked by the scan
        const float *anp = a.anc + (int64_t)an * 7 * HW + cell;
        const float *rp = r + (int64_t)(7 * an) * HW + cell;
        const float *box = bx + (int64_t)k * a.box_stride;
        double A[7], R[7], q[7], p[7], chain[7], gp[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) { A[c] = (double)anp[(int64_t)c * HW]; R[c] = (double)rp[(int64_t)c * HW]; q[c] = (double)box[c]; }
        const double diag = sqrt(A[3] * A[3] + A[4] * A[4]);
        p[0] = R[0] * diag + A[0];
        p[1] = R[1] * diag + A[1];
        p[2] = R[2] * A[5] + A[2];
        p[3] = exp(R[3]) * A[3];
        p[4] = exp(R[4]) * A[4];
        p[5] = exp(R[5]) * A[5];
        p[6] = R[6] + A[6];
        chain[0] = diag; chain[1] = diag; chain[2] = A[5]; chain[3] = p[3]; chain[4] = p[4]; chain[5] = p[5]; chain[6] = 1.0;
        const double iou = il_pair(p, q, a.kind, gp);
        s_iou[i] = iou;
        if (map) map[j] = iou;
        float *gq = gr + (int64_t)(7 * an) * HW + cell;
#pragma unroll
        for (int c = 0; c < 7; ++c) gq[(int64_t)c * HW] += (float)(gscale * (gp[c] * chain[c]));
    }
    __syncthreads();
    if (tid == 0) {
        double s1 = 0.0, s = 0.0;
        for (int i = 0; i < cnt; ++i) { s1 += 1.0 - s_iou[i]; s += s_iou[i]; }
        double *slot = a.ws + ((int64_t)b * a.G + g) * 2;
        slot[0] = s1; slot[1] = s;
    }
}

// One wave: per sample the slots added in a fixed order in double (lane l takes g = l, l + 64, ..., then a butterfly: every lane ends with
// the same bits), loss[0] += sum_b wsample gain s1_b / max(1, N_b), rounded once; terms [B][2] = (sum of IoU / max(1, N_b), N_b), zero rows
// for the samples 'last' leaves out.
__global__ void __launch_bounds__(64) k_loss_anchor_iou_fold(const double *ws, const int32_t *counts, int B, int b0, int G, float gain,
                                                             float wsample, float *loss, float *terms)
{
    const int lane = threadIdx.x;
    double tot = 0.0;
    for (int b = 0; b < B; ++b) {
        if (b < b0) {
            if (lane == 0) { terms[2 * b] = 0.f; terms[2 * b + 1] = 0.f; }
            continue;
        }
        double s1 = 0.0, s = 0.0;
        for (int g = lane; g < G; g += 64) {
            const double *slot = ws + ((int64_t)b * G + g) * 2;
            s1 += slot[0]; s += slot[1];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s += __shfl_xor(s, o, 64); }
        const int n = counts[4 * b];
        const double den = (double)max(n, 1);
        if (lane == 0) { terms[2 * b] = (float)(s / den); terms[2 * b + 1] = (float)n; }
        tot += (double)wsample * (double)gain * (s1 / den);
    }
    if (lane == 0) *loss = (float)((double)*loss + tot);
}

int il_groups(int H, int W) { return cdiv(2 * (int64_t)H * W, IL_CHUNK); }

}  // namespace

extern "C" size_t dcf_loss_anchor_iou_workspace_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W >= (int64_t)1 << 30) return 0;
    return (size_t)B * il_groups(H, W) * 2 * sizeof(double);
}

extern "C" int dcf_loss_anchor_iou_fwd_bwd(const float *reg, int64_t reg_bstride, const float *anchors, const float *boxes, int max_box,
                                           int box_stride, const int32_t *target, const int32_t *counts, int B, int H, int W, int kind,
                                           float iou_gain, int reduction, float *loss, float *greg, int64_t greg_bstride, float *iou_terms,
                                           double *iou_map, void *workspace, dcf_stream_t stream)
{
    DCF_REQUIRE(reg && anchors && boxes && target && counts && loss && greg && iou_terms && B > 0 && H > 0 && W > 0,
                "dcf_loss_anchor_iou_fwd_bwd: bad arguments");
    DCF_REQUIRE(reduction >= 0 && reduction <= 2, "dcf_loss_anchor_iou_fwd_bwd: reduction must be 0 (last), 1 (sum) or 2 (mean)");
    DCF_REQUIRE(kind == 0 || kind == 1, "dcf_loss_anchor_iou_fwd_bwd: kind must be 0 (3-D) or 1 (bird's-eye)");
    DCF_REQUIRE(max_box >= 1 && max_box <= 64 && box_stride >= 7, "dcf_loss_anchor_iou_fwd_bwd: 1 to 64 boxes per sample, at least 7 values each");
    DCF_REQUIRE((int64_t)H * W < (int64_t)1 << 30, "dcf_loss_anchor_iou_fwd_bwd: map too large");
    DCF_REQUIRE(iou_gain >= 0.f && iou_gain <= 3.0e38f, "dcf_loss_anchor_iou_fwd_bwd: the gain must be finite and not negative");
    DCF_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)iou_map & 7) == 0,
                "dcf_loss_anchor_iou_fwd_bwd: null or misaligned workspace / iou_map");
    IouArgs a;
    a.reg = reg; a.anc = anchors; a.boxes = boxes; a.target = target; a.counts = counts;
    a.reg_bs = reg_bstride; a.greg_bs = greg_bstride; a.greg = greg;
    a.ws = (double *)workspace; a.iou_map = iou_map;
    a.max_box = max_box; a.box_stride = box_stride; a.B = B; a.HW = H * W; a.kind = kind; a.reduction = reduction;
    a.b0 = reduction == 0 ? B - 1 : 0;              // 'last': only the last sample is computed
    a.G = il_groups(H, W);
    a.gain = iou_gain;
    hipStream_t s = S(stream);
    DCF_LAUNCH_B("loss_anchor_iou", (double)(B - a.b0) * a.HW * 2.0 * 4.0, s,
                 hipLaunchKernelGGL(k_loss_anchor_iou, dim3(a.G, B - a.b0), dim3(IL_THREADS), 0, s, a));
    DCF_LAUNCH("loss_anchor_iou_fold", s, hipLaunchKernelGGL(k_loss_anchor_iou_fold, dim3(1), dim3(64), 0, s, a.ws, counts, B, a.b0, a.G,
                                                              iou_gain, il_sample_weight(reduction, B), loss, iou_terms));
    return DCF_OK;
}
