// loss.hip -- the device half of the detection objective (loss.py:129-189 of the reference).
// (Further down: the device sampler, hard negative mining, the dense focal term and the IoU-based anchor assignment.)
//
// Target assignment stays on the host (it consumes numpy's global RNG exactly like loss.py:74-127); what runs here is
// everything that touches the head outputs: the 2-way cross-entropy at the sampled positive / negative cells of both
// anchors (mean per list, loss.py:129-142), the Smooth-L1 of the encoded box offsets at the regression cells
// (loss.py:144-186) -- and their gradients, written straight into dense gradient maps.  One launch replaces the ~60 tiny
// gather / softmax / index_put kernels of the vectorised torch version.
#include "dcf_common.h"
#include "ev_geom.h"        // the evaluation's fp64 rectangle clip: the anchor assignment's IoU

namespace {

// the sum of v over a workgroup of NWAVES waves (4 or 16), in a fixed order
template <int NWAVES>
__device__ __forceinline__ float block_sum(float v, float *red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if constexpr (NWAVES == 4) return (red[0] + red[1]) + (red[2] + red[3]);
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < NWAVES / 4; ++q) t += (red[4 * q] + red[4 * q + 1]) + (red[4 * q + 2] + red[4 * q + 3]);
    return t;
}

// encoded regression target of component j of a box against the anchor at a cell (an = anchor parameters of the cell, HW apart)
__device__ __forceinline__ float reg_target(const float *bx, const float *an, int j, int HW)
{
    if (j < 2) {
        const float l = an[3 * HW], w = an[4 * HW];
        return (bx[j] - an[j * HW]) / sqrtf(l * l + w * w);
    }
    if (j == 2) return (bx[2] - an[2 * HW]) / an[5 * HW];
    if (j < 6) return logf(bx[j] / an[j * HW]);
    const float d = bx[6] - an[6 * HW];
    return atan2f(sinf(d), cosf(d));
}
__device__ __forceinline__ float sl1_grad(float d) { return fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : -1.f); }

// ---------------------------------------------------------------------------------------------------------------------
// The terms of one sample, written once for both kernels of this file.  The kernels differ only in where a list item comes from,
// so each hands the code below an accessor (ListItems / SampledItems, beside their kernels) that answers
//   npos, nneg, cell(j)     the classification list: item j < npos is a positive, the others are negatives
//   nrows, row_cell(r), row_counts(r), row_weight(r), row_box(r)     the regression rows (a row that does not count has no term)
//
// DET (deterministic: true): a cell can occur several times in a sample's lists (overlapping positive windows,
// negatives drawn with replacement), and three or more float atomics onto one address do not commute.  There the FIRST entry of a
// cell adds the terms of all entries of that cell in list order and stores the sum once; the sample's loss value goes to its own
// slot of loss_rows (k_loss_rows_fold adds the slots in sample order).  The lists hold a few hundred entries: the scans are cheap.
struct SampleMaps {
    const float *c, *r, *anc;       // the sample's scores [4][HW] and offsets [14][HW]; the anchors [2][7][HW]
    float *gc, *gr;                 // the sample's gradient maps
    int HW;
    float gain, wsample;
};

// reduction 0 = 'last' (reference behaviour: only the last sample counts), 1 = 'sum', 2 = 'mean'
__host__ __device__ __forceinline__ float sample_weight(int reduction, int B) { return reduction == 2 ? 1.f / (float)B : 1.f; }

// false for a sample that 'last' leaves out: its workgroup has nothing more to do
template <bool DET>
__device__ __forceinline__ bool sample_counts(int reduction, int b, int B, float *loss_rows)
{
    if (reduction != 0 || b == B - 1) return true;
    if constexpr (DET) {
        // DCF-DET-BEGIN
        if (threadIdx.x == 0) loss_rows[b] = 0.f;
        // DCF-DET-END
    }
    return false;
}

// 2-way cross-entropy, entry e = (anchor a, list item): mean per list (loss.py:129-142)
template <bool DET, class Items>
__device__ __forceinline__ void cls_entry(const Items &L, const SampleMaps &m, int e, float &acc)
{
    const int npos = L.npos, nneg = L.nneg, HW = m.HW;
    const int a = e / (npos + nneg), it = e - a * (npos + nneg);
    const bool is_pos = it < npos;
    const int cell = L.cell(it);
    const float inv = 1.f / (float)(is_pos ? npos : nneg);
    const float s0 = m.c[(int64_t)(2 * a) * HW + cell], s1 = m.c[(int64_t)(2 * a + 1) * HW + cell];
    const float mx = fmaxf(s0, s1);
    const float e0 = expf(s0 - mx), e1 = expf(s1 - mx);
    const float lse = mx + logf(e0 + e1);
    const float p0 = e0 / (e0 + e1), p1 = e1 / (e0 + e1);
    acc += (lse - (is_pos ? s1 : s0)) * inv;
    if constexpr (DET) {
        // DCF-DET-BEGIN
        const int nl = npos + nneg;
        bool first = true;
        for (int j = 0; j < it && first; ++j) first = L.cell(j) != cell;
        if (first) {
            float g0 = 0.f, g1 = 0.f;
            for (int j = it; j < nl; ++j) {
                if (L.cell(j) != cell) continue;
                const bool jp = j < npos;
                const float gj = (1.f / (float)(jp ? npos : nneg)) * m.wsample;
                g0 += (p0 - (jp ? 0.f : 1.f)) * gj;
                g1 += (p1 - (jp ? 1.f : 0.f)) * gj;
            }
            m.gc[(int64_t)(2 * a) * HW + cell] += g0;
            m.gc[(int64_t)(2 * a + 1) * HW + cell] += g1;
        }
        // DCF-DET-END
    } else {
        const float g = inv * m.wsample;
        atomicAdd(m.gc + (int64_t)(2 * a) * HW + cell, (p0 - (is_pos ? 0.f : 1.f)) * g);
        atomicAdd(m.gc + (int64_t)(2 * a + 1) * HW + cell, (p1 - (is_pos ? 1.f : 0.f)) * g);
    }
}

// Smooth-L1 of the encoded box offsets, entry e = (row, anchor a, component j) (loss.py:144-186)
template <bool DET, class Items>
__device__ __forceinline__ void reg_entry(const Items &L, const SampleMaps &m, int e, float &accr)
{
    const int row = e / 14, q = e - row * 14;
    if (!L.row_counts(row)) return;
    const int a = q / 7, j = q - a * 7, HW = m.HW;
    const int cell = L.row_cell(row);
    const float wrow = L.row_weight(row);
    const float *an = m.anc + (int64_t)a * 7 * HW + cell;     // an[j * HW]
    const float t = reg_target(L.row_box(row), an, j, HW);
    const float d = m.r[(int64_t)q * HW + cell] - t;
    const float ad = fabsf(d);
    accr += (ad < 1.f ? 0.5f * d * d : ad - 0.5f) * wrow;
    if constexpr (DET) {
        // DCF-DET-BEGIN
        bool first = true;
        for (int r2 = 0; r2 < row && first; ++r2) first = !(L.row_cell(r2) == cell && L.row_counts(r2));
        if (first) {
            float gs = 0.f;
            for (int r2 = row; r2 < L.nrows; ++r2) {
                if (L.row_cell(r2) != cell || !L.row_counts(r2)) continue;
                const float d2 = m.r[(int64_t)q * HW + cell] - reg_target(L.row_box(r2), an, j, HW);
                gs += sl1_grad(d2) * L.row_weight(r2) * m.gain * m.wsample;
            }
            m.gr[(int64_t)q * HW + cell] += gs;
        }
        // DCF-DET-END
    } else {
        atomicAdd(m.gr + (int64_t)q * HW + cell, (ad < 1.f ? d : (d > 0.f ? 1.f : -1.f)) * wrow * m.gain * m.wsample);
    }
}

// every entry of sample b over the workgroup's NWAVES waves, then the sample's value
template <bool DET, int NWAVES, class Items>
__device__ __forceinline__ void sample_terms(const Items &L, const SampleMaps &m, int b, float *red, float *loss, float *loss_rows)
{
    float acc = 0.f, accr = 0.f;
    for (int e = threadIdx.x; e < 2 * (L.npos + L.nneg); e += blockDim.x) cls_entry<DET>(L, m, e, acc);
    for (int e = threadIdx.x; e < L.nrows * 14; e += blockDim.x) reg_entry<DET>(L, m, e, accr);
    const float tot = block_sum<NWAVES>(acc + m.gain * accr, red);
    if constexpr (DET) {
        // DCF-DET-BEGIN
        if (threadIdx.x == 0) loss_rows[b] = tot * m.wsample;
        // DCF-DET-END
    } else {
        if (threadIdx.x == 0) atomicAdd(loss, tot * m.wsample);
    }
}

// The lists of the host's target assignment:
// ints  = [B x {off_int, npos, nneg, nrow, off_float, nbox}] then per sample: pos cells, neg cells, reg cells, box of each reg cell
// floats = per sample: weight of each reg cell, then nbox x 7 box parameters
struct ListItems {
    const int64_t *pos, *neg, *rows, *rbox;
    const float *wrow, *boxes;
    const int *lcell, *lrow;        // DET: the cells of the two lists staged in LDS (the scans read them often), or null
    int npos, nneg, nrows;
    __device__ __forceinline__ int cell(int j) const { return lcell ? lcell[j] : (int)(j < npos ? pos[j] : neg[j - npos]); }
    __device__ __forceinline__ int row_cell(int r) const { return lrow ? lrow[r] : (int)rows[r]; }
    __device__ __forceinline__ bool row_counts(int) const { return true; }
    __device__ __forceinline__ float row_weight(int r) const { return wrow[r]; }
    __device__ __forceinline__ const float *row_box(int r) const { return boxes + (int64_t)rbox[r] * 7; }
};

// (1024 threads: with the reference's 'last' reduction ONE workgroup does all the work, and its entries are chains of dependent
// loads -- list item -> cell -> scores -> atomics; at 256 threads the launch took 40 us between forward and backward)
template <bool DET>
__global__ void __launch_bounds__(1024) k_loss_fwd_bwd(const float *cls, int64_t cls_bs, const float *reg, int64_t reg_bs, const float *anc,
                                                      const int64_t *ints, const float *floats, int B, int HW, float gain, int reduction,
                                                      float *loss, float *gcls, int64_t gcls_bs, float *greg, int64_t greg_bs, float *loss_rows)
{
    __shared__ float red[16];
    const int b = blockIdx.x;
    if (!sample_counts<DET>(reduction, b, B, loss_rows)) return;
    const int64_t *pl = ints + 6 * b;
    const int o = (int)pl[0], of = (int)pl[4];
    ListItems L;
    L.npos = (int)pl[1]; L.nneg = (int)pl[2]; L.nrows = (int)pl[3];
    L.pos = ints + o; L.neg = L.pos + L.npos; L.rows = L.neg + L.nneg; L.rbox = L.rows + L.nrows;
    L.wrow = floats + of; L.boxes = L.wrow + L.nrows;
    L.lcell = nullptr; L.lrow = nullptr;
    if constexpr (DET) {
        // DCF-DET-BEGIN
        constexpr int MAXL = 2048;      // longer lists are scanned in global memory
        __shared__ int s_cell[MAXL], s_row[MAXL];
        if (L.npos + L.nneg <= MAXL) {
            for (int i = threadIdx.x; i < L.npos + L.nneg; i += blockDim.x) s_cell[i] = L.cell(i);
            L.lcell = s_cell;
        }
        if (L.nrows <= MAXL) {
            for (int i = threadIdx.x; i < L.nrows; i += blockDim.x) s_row[i] = L.row_cell(i);
            L.lrow = s_row;
        }
        __syncthreads();
        // DCF-DET-END
    }
    const SampleMaps m = {cls + b * cls_bs, reg + b * reg_bs, anc, gcls + b * gcls_bs, greg + b * greg_bs, HW, gain, sample_weight(reduction, B)};
    sample_terms<DET, 16>(L, m, b, red, loss, loss_rows);
}

// *loss += rows[0] + rows[1] + ... in sample order
__global__ void k_loss_rows_fold(const float *rows, int n, float *loss)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float tot = 0.f;
    for (int i = 0; i < n; ++i) tot += rows[i];
    *loss += tot;
}

// ---------------------------------------------------------------------------------------------------------------------
// Device-side target assignment ("sampling: device"): loss.py:74-127 without the host -- the positive
// windows of the labelled boxes, a random subset of them when there are more than pos_cap, neg_count random cells that are
// not selected positives -- followed by the same loss terms as above, in ONE launch (one workgroup per sample).
//
// Randomness is a counter-based hash of (seed, sample, stream, index, attempt): no state, no order dependence, the same lists
// for the same seed on every launch -- tests/test_gpu_loss_sampling.py restates it in Python and compares the lists bit for
// bit.  Semantics kept from the reference: the positive list has one entry per (box, window cell) (overlapping windows give a
// cell twice), the subset is uniform without replacement over ENTRIES (loss.py:107-110: shuffle, truncate), negatives are
// drawn with replacement and rejected only against the selected positives (loss.py:117-126).
// (dcf_mix64: dcf_common.h -- the point-drop hash of csrc/geometry.hip is the same function)
__host__ __device__ inline uint32_t dcf_loss_rand(uint64_t seed, int sample, int stream, int index, int attempt)
{
    const uint64_t ctr = ((uint64_t)(uint32_t)sample << 44) | ((uint64_t)(uint32_t)stream << 40) | ((uint64_t)(uint32_t)attempt << 20) | (uint64_t)(uint32_t)index;
    return (uint32_t)(dcf_mix64(seed ^ dcf_mix64(ctr)) >> 32);
}

constexpr int LS_MAXE = 1024;       // positive entries per sample (max_box * span^2)
constexpr int LS_MAXNEG = 512;

// ---------------------------------------------------------------------------------------------------------------------
// Hard negative mining ("loss_sampling: hard"): the negatives of a sample are the neg_count cells outside
// every positive window with the highest key, key(cell) = max over the two anchors of ord(s1 - s0) -- ord = the order-preserving
// map from fp32 to unsigned, so everything below is integer work and agrees with the host statement (loss.py, hard_negatives)
// bit for bit.  Window cells get key 0 and candidates at least 1 (the two keys that moves are NaN patterns), so "k-th largest
// over the whole map" never lands on a window cell while k <= number of candidates.
//
// An exact radix select, 8 bits per pass, G workgroups per sample over contiguous chunks of the map:
//   k_hard_keys          keys -> workspace, per-workgroup histogram of the top digit, per-workgroup candidate count
//   k_hard_pass  x 3     every workgroup folds the G histograms of the pass before, finds the digit that holds the k-th largest
//                        key, and builds its histogram of the next digit over the cells that match the prefix so far
//   k_hard_compact       last digit -> the cut key; cells above it go to the list through an integer cursor (their order is
//                        settled later), of the cells equal to it the r lowest-index ones: a workgroup knows how many ties the
//                        chunks before its own hold from their histograms, and walks its own chunk in order
//   k_loss_sample_fwd_bwd<DET, true>  ranks the <= 512 survivors by (key descending, cell ascending) and does the terms
// Histograms are built with integer LDS atomics and STORED per workgroup, never merged with global atomics: nothing here depends
// on scheduling, and the workspace needs no clearing between calls (the cursor is reset by k_hard_keys).
//
// per-sample workspace, in ints:
constexpr int HS_CURSOR = 0;                    // list cursor of the cells above the cut
constexpr int HS_STATE = 1;                     // (prefix, k remaining) after pass 1, 2, 3: 6 ints
constexpr int HS_K = 7;                         // nneg = min(neg_count, candidates)
constexpr int HS_CNT = 16;                      // candidates per workgroup [HARD_MAXG]
constexpr int HARD_MAXG = 64;
constexpr int HS_LIST = HS_CNT + HARD_MAXG;     // survivors [LS_MAXNEG]
constexpr int HS_HIST = HS_LIST + LS_MAXNEG;    // two sets of [HARD_MAXG][256] histograms, used in turn
constexpr int HS_KEYS = HS_HIST + 2 * HARD_MAXG * 256;      // keys [HW]
constexpr int HARD_THREADS = 256;

__host__ __device__ inline int64_t hard_ws_stride(int HW) { return ((int64_t)HS_KEYS + HW + 3) & ~(int64_t)3; }
// cells per workgroup: a multiple of the workgroup, at least 1024, and no more than HARD_MAXG chunks per sample
__host__ __device__ inline int hard_chunk(int HW)
{
    const int per = (HW + HARD_MAXG - 1) / HARD_MAXG;
    const int up = (per + HARD_THREADS - 1) / HARD_THREADS * HARD_THREADS;
    return up > 1024 ? up : 1024;
}

__device__ __forceinline__ unsigned hard_ord(float d)
{
    const unsigned u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}

struct HardArgs {
    const float *cls, *boxes;
    const int32_t *nbox;
    int64_t cls_bs, ws_stride;
    int32_t *ws;
    int max_box, box_stride, b0, H, W, span, neg_count, G, chunk;
    float xs, xo, ys, yo, rs;
};

// Folds the G per-workgroup histograms at `hist` and finds the digit d with count(digit > d) < kr <= count(digit >= d); returns d and
// leaves kr - count(digit > d) in *kr_out.  kr == 0 (no candidates): digit 0, kr 0.  All HARD_THREADS threads call it.
__device__ __forceinline__ int hard_pick_digit(const int32_t *hist, int G, int kr, int *s_suf, int *s_pick, int *kr_out)
{
    const int t = threadIdx.x;
    int tot = 0;
    for (int g = 0; g < G; ++g) tot += hist[g * 256 + t];
    if (t == 0) { s_pick[0] = 0; s_pick[1] = 0; }
    s_suf[t] = tot;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {                     // s_suf[t] = count(digit >= t)
        const int v = t + off < 256 ? s_suf[t + off] : 0;
        __syncthreads();
        s_suf[t] += v;
        __syncthreads();
    }
    const int above = t + 1 < 256 ? s_suf[t + 1] : 0;
    if (kr > 0 && s_suf[t] >= kr && above < kr) { s_pick[0] = t; s_pick[1] = kr - above; }      // (one thread at most: s_suf falls with t)
    __syncthreads();
    *kr_out = s_pick[1];
    return s_pick[0];
}

__global__ void __launch_bounds__(HARD_THREADS) k_hard_keys(HardArgs a)
{
    __shared__ int hist[256];
    __shared__ int box_cx[64], box_cy[64];
    __shared__ int s_cnt;
    const int g = blockIdx.x, b = a.b0 + blockIdx.y, tid = threadIdx.x;
    const int HW = a.H * a.W, half = a.span / 2;
    const int nb = min(a.nbox[b], a.max_box);
    const float *bx = a.boxes + (int64_t)b * a.max_box * a.box_stride;
    int32_t *ws = a.ws + (int64_t)b * a.ws_stride;
    hist[tid] = 0;
    if (tid == 0) s_cnt = 0;
    if (tid < nb) {
        // the centre cell exactly as k_loss_sample_fwd_bwd computes it; a box outside the map has no window
        const int cx = (int)(__fdiv_rn(__fadd_rn(__fmul_rn(bx[tid * a.box_stride], a.xs), a.xo), a.rs));
        const int cy = (int)(__fdiv_rn(__fadd_rn(__fmul_rn(bx[tid * a.box_stride + 1], a.ys), a.yo), a.rs));
        const bool in = !(cx < 0 || cx > a.H - 1 || cy < 0 || cy > a.W - 1);
        box_cx[tid] = in ? cx : -1000000; box_cy[tid] = in ? cy : 0;
    }
    __syncthreads();
    const float *c = a.cls + b * a.cls_bs;
    unsigned *keys = (unsigned *)(ws + HS_KEYS);
    const int lo = g * a.chunk, hi = min(lo + a.chunk, HW);
    int cnt = 0;
    for (int cell = lo + tid; cell < hi; cell += HARD_THREADS) {
        const int px = cell / a.W, py = cell - px * a.W;
        bool window = false;
        for (int k = 0; k < nb; ++k) {
            const int dx = px - (box_cx[k] - half), dy = py - (box_cy[k] - half);
            window |= dx >= 0 && dx < a.span && dy >= 0 && dy < a.span;
        }
        unsigned key = 0;
        if (!window) {
            const unsigned k0 = hard_ord(__fsub_rn(c[(int64_t)HW + cell], c[cell]));
            const unsigned k1 = hard_ord(__fsub_rn(c[(int64_t)3 * HW + cell], c[(int64_t)2 * HW + cell]));
            key = max(max(k0, k1), 1u);
            ++cnt;
        }
        keys[cell] = key;
        atomicAdd(&hist[key >> 24], 1);
    }
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    ws[HS_HIST + g * 256 + tid] = hist[tid];
    if (tid == 0) {
        ws[HS_CNT + g] = s_cnt;
        if (g == 0) ws[HS_CURSOR] = 0;
    }
}

// pass p = 1, 2, 3 (digit shift 24 - 8p)
__global__ void __launch_bounds__(HARD_THREADS) k_hard_pass(HardArgs a, int p)
{
    __shared__ int hist[256], s_suf[256];
    __shared__ int s_pick[2];
    const int g = blockIdx.x, b = a.b0 + blockIdx.y, tid = threadIdx.x;
    const int HW = a.H * a.W;
    int32_t *ws = a.ws + (int64_t)b * a.ws_stride;
    unsigned prefix = 0;
    int kr;
    if (p == 1) {
        int ncand = 0;
        for (int i = 0; i < a.G; ++i) ncand += ws[HS_CNT + i];
        kr = min(a.neg_count, ncand);
    } else {
        prefix = (unsigned)ws[HS_STATE + 2 * (p - 2)];
        kr = ws[HS_STATE + 2 * (p - 2) + 1];
    }
    hist[tid] = 0;
    const int shift = 24 - 8 * p;
    const int d = hard_pick_digit(ws + HS_HIST + ((p - 1) & 1) * HARD_MAXG * 256, a.G, kr, s_suf, s_pick, &kr);
    prefix |= (unsigned)d << (shift + 8);
    if (g == 0 && tid == 0) { ws[HS_STATE + 2 * (p - 1)] = (int)prefix; ws[HS_STATE + 2 * (p - 1) + 1] = kr; }
    const unsigned *keys = (const unsigned *)(ws + HS_KEYS);
    const int lo = g * a.chunk, hi = min(lo + a.chunk, HW);
    for (int cell = lo + tid; cell < hi; cell += HARD_THREADS) {
        const unsigned key = keys[cell];
        if ((key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u], 1);
    }
    __syncthreads();
    ws[HS_HIST + (p & 1) * HARD_MAXG * 256 + g * 256 + tid] = hist[tid];
}

__global__ void __launch_bounds__(HARD_THREADS) k_hard_compact(HardArgs a)
{
    __shared__ int s_suf[256];
    __shared__ int s_pick[2];
    __shared__ int s_wave[HARD_THREADS / 64];
    const int g = blockIdx.x, b = a.b0 + blockIdx.y, tid = threadIdx.x;
    const int HW = a.H * a.W;
    int32_t *ws = a.ws + (int64_t)b * a.ws_stride;
    const int32_t *hist = ws + HS_HIST + HARD_MAXG * 256;          // pass 3's histograms: the last digit of the cells that match 24 bits
    int r;
    const int d = hard_pick_digit(hist, a.G, ws[HS_STATE + 5], s_suf, s_pick, &r);
    const unsigned cut = (unsigned)ws[HS_STATE + 4] | (unsigned)d;
    int ncand = 0;
    for (int i = 0; i < a.G; ++i) ncand += ws[HS_CNT + i];
    const int k = min(a.neg_count, ncand);
    if (g == 0 && tid == 0) ws[HS_K] = k;
    if (k == 0) return;
    const int above = k - r;                        // cells with a key above the cut: slots [0, above) through the cursor
    int tie_base = 0;                               // ties in the chunks before this one
    for (int i = 0; i < g; ++i) tie_base += hist[i * 256 + d];
    const unsigned *keys = (const unsigned *)(ws + HS_KEYS);
    int32_t *list = ws + HS_LIST;
    const int lo = g * a.chunk, hi = min(lo + a.chunk, HW);
    for (int t0 = lo; t0 < hi; t0 += HARD_THREADS) {               // tiles in cell order
        const int cell = t0 + tid;
        const unsigned key = cell < hi ? keys[cell] : 0u;          // (cut >= 1: key 0 is neither above nor a tie)
        if (key > cut) {
            const int slot = atomicAdd(&ws[HS_CURSOR], 1);
            if (slot < above) list[slot] = cell;
        }
        const bool tie = key == cut;
        const unsigned long long m = __ballot(tie);
        const int lane = tid & 63, wv = tid >> 6;
        __syncthreads();                                           // (s_wave of the tile before has been read)
        if (lane == 0) s_wave[wv] = __popcll(m);
        __syncthreads();
        int before = tie_base + __popcll(m & ((1ull << lane) - 1ull));
        int tile_ties = 0;
        for (int w = 0; w < HARD_THREADS / 64; ++w) {
            if (w < wv) before += s_wave[w];
            tile_ties += s_wave[w];
        }
        if (tie && before < r) list[above + before] = cell;
        tie_base += tile_ties;
    }
}

struct LossSampleArgs {
    const float *cls, *reg, *anc, *boxes;
    const int32_t *nbox;
    int64_t cls_bs, reg_bs, gcls_bs, greg_bs;
    float *loss, *gcls, *greg, *loss_rows;
    int32_t *pos_out, *neg_out, *counts_out;
    uint64_t seed;
    int max_box, box_stride, B, H, W, span, regress_type, pos_cap, neg_count, reduction;
    float xs, xo, ys, yo, rs, gain;
    // loss_sampling: hard -- the mined negatives of samples >= hard_b0 wait in the workspace (k_hard_* below)
    const int32_t *hard_ws;
    int64_t hard_stride;
    int hard_b0;
};

// The lists the sample kernel leaves in LDS: selected positives, negatives, and the window entries as regression rows -- every entry
// (regress_type 0) or the centre cell only; a box's rows share its weight 1 / (rows * 14)
struct SampledItems {
    const int *sel, *negs, *e_cell;
    const short *e_box;
    const int *box_first, *box_cx, *box_cy;
    const float *bx;                // the sample's boxes, box_stride apart
    int box_stride, regress_type, W;
    int npos, nneg, nrows;
    __device__ __forceinline__ int cell(int j) const { return j < npos ? sel[j] : negs[j - npos]; }
    __device__ __forceinline__ int row_cell(int r) const { return e_cell[r]; }
    __device__ __forceinline__ bool row_counts(int r) const { return regress_type == 0 || e_cell[r] == box_cx[e_box[r]] * W + box_cy[e_box[r]]; }
    __device__ __forceinline__ float row_weight(int r) const
    {
        const int k = e_box[r];
        return 1.f / (float)((regress_type != 0 ? 1 : box_first[k + 1] - box_first[k]) * 14);
    }
    __device__ __forceinline__ const float *row_box(int r) const { return bx + (int64_t)e_box[r] * box_stride; }
};

template <bool DET, bool HARD = false>
__global__ void __launch_bounds__(256) k_loss_sample_fwd_bwd(LossSampleArgs a)
{
    __shared__ float red[4];
    __shared__ int e_cell[LS_MAXE];            // entry -> cell (px * W + py)
    __shared__ short e_box[LS_MAXE];           // entry -> box
    __shared__ unsigned e_key[LS_MAXE];
    __shared__ int sel[LS_MAXE];               // selected positive cells (compacted, entry order)
    __shared__ int negs[LS_MAXNEG];
    __shared__ int box_first[65], box_cx[64], box_cy[64];
    __shared__ int s_np, s_nsel;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int HW = a.H * a.W, half = a.span / 2;
    int nneg = a.neg_count;
    const int nb = min(a.nbox[b], a.max_box);
    const float *bx = a.boxes + (int64_t)b * a.max_box * a.box_stride;
    // ---- positive entries: box k's window cells inside the map, in the reference's order (box, dx, dy)
    if (tid == 0) {
        int n = 0;
        for (int k = 0; k < nb; ++k) {
            // fp32 arithmetic and truncation as the reference does on 0-dim tensors (loss.py:85-86)
            const int cx = (int)(__fdiv_rn(__fadd_rn(__fmul_rn(bx[k * a.box_stride], a.xs), a.xo), a.rs));
            const int cy = (int)(__fdiv_rn(__fadd_rn(__fmul_rn(bx[k * a.box_stride + 1], a.ys), a.yo), a.rs));
            box_first[k] = n;
            box_cx[k] = cx; box_cy[k] = cy;
            if (cx < 0 || cx > a.H - 1 || cy < 0 || cy > a.W - 1) { box_cx[k] = -1000000; continue; }
            for (int dx = 0; dx < a.span; ++dx)
                for (int dy = 0; dy < a.span; ++dy) {
                    const int px = cx - half + dx, py = cy - half + dy;
                    if (px < 0 || px > a.H - 1 || py < 0 || py > a.W - 1) continue;
                    if (n < LS_MAXE) { e_cell[n] = px * a.W + py; e_box[n] = (short)k; }
                    ++n;
                }
        }
        box_first[nb] = n;
        s_np = min(n, LS_MAXE);
    }
    __syncthreads();
    const int np = s_np;
    // ---- subset of pos_cap entries when there are more: the pos_cap smallest (key, entry) pairs
    for (int i = tid; i < np; i += blockDim.x) e_key[i] = dcf_loss_rand(a.seed, b, 1, i, 0);
    __syncthreads();
    const bool cut = np > a.pos_cap;
    for (int i = tid; i < np; i += blockDim.x) {
        bool keep = true;
        if (cut) {
            int rank = 0;
            const unsigned ki = e_key[i];
            for (int j = 0; j < np; ++j) rank += (e_key[j] < ki || (e_key[j] == ki && j < i)) ? 1 : 0;
            keep = rank < a.pos_cap;
        }
        sel[i] = keep ? 1 : 0;                   // (flags first: the keys are still being read by other threads)
    }
    __syncthreads();
    if (tid == 0) {                              // order-preserving compaction in place (<= 1024 entries: a serial scan is microseconds)
        int n = 0;
        for (int i = 0; i < np; ++i)
            if (sel[i]) sel[n++] = e_cell[i];    // n <= i: the flag of entry i is read before slot n is written
        s_nsel = n;
    }
    __syncthreads();
    const int npos = s_nsel;
    if constexpr (HARD) {
        // ---- negatives: the survivors of the selection (k_hard_compact), here put in order: key descending, then cell ascending
        __shared__ unsigned n_key[LS_MAXNEG];
        __shared__ int n_cell[LS_MAXNEG];
        nneg = 0;
        if (b >= a.hard_b0) {
            const int32_t *ws = a.hard_ws + (int64_t)b * a.hard_stride;
            nneg = min(min(ws[HS_K], a.neg_count), LS_MAXNEG);
            const unsigned *keys = (const unsigned *)(ws + HS_KEYS);
            for (int i = tid; i < nneg; i += blockDim.x) {
                const int cell = min(max(ws[HS_LIST + i], 0), HW - 1);      // (every slot below k is filled: count(> cut) + ties taken = k)
                n_cell[i] = cell;
                n_key[i] = keys[cell];
                negs[i] = cell;
            }
            __syncthreads();
            for (int i = tid; i < nneg; i += blockDim.x) {
                int rank = 0;
                const unsigned ki = n_key[i];
                const int ci = n_cell[i];
                for (int j = 0; j < nneg; ++j) rank += (n_key[j] > ki || (n_key[j] == ki && n_cell[j] < ci)) ? 1 : 0;
                negs[rank] = ci;
            }
        }
    } else {
        // ---- negatives: item i keeps drawing until its cell is not a selected positive
        for (int i = tid; i < a.neg_count; i += blockDim.x) {
            int cell = 0;
            for (int att = 0; att < (1 << 20); ++att) {
                const uint32_t u = dcf_loss_rand(a.seed, b, 2, i, att);
                cell = (int)(((uint64_t)u * (uint64_t)HW) >> 32);
                bool hit = false;
                for (int j = 0; j < npos; ++j) hit |= sel[j] == cell;
                if (!hit) break;
            }
            negs[i] = cell;
        }
    }
    __syncthreads();
    if (a.pos_out)
        for (int i = tid; i < a.pos_cap; i += blockDim.x) a.pos_out[(int64_t)b * a.pos_cap + i] = i < npos ? sel[i] : -1;
    if (a.neg_out)
        for (int i = tid; i < a.neg_count; i += blockDim.x) a.neg_out[(int64_t)b * a.neg_count + i] = i < nneg ? negs[i] : -1;
    if (a.counts_out && tid == 0) {
        constexpr int NC = HARD ? 3 : 2;
        a.counts_out[NC * b] = npos; a.counts_out[NC * b + 1] = np;
        if constexpr (HARD) a.counts_out[NC * b + 2] = nneg;
    }
    if (!sample_counts<DET>(a.reduction, b, a.B, a.loss_rows)) return;
    const SampledItems L = {sel, negs, e_cell, e_box, box_first, box_cx, box_cy, bx, a.box_stride, a.regress_type, a.W, npos, nneg, np};
    const SampleMaps m = {a.cls + b * a.cls_bs, a.reg + b * a.reg_bs, a.anc, a.gcls + b * a.gcls_bs, a.greg + b * a.greg_bs, HW, a.gain,
                          sample_weight(a.reduction, a.B)};
    sample_terms<DET, 4>(L, m, b, red, a.loss, a.loss_rows);
}

// ---------------------------------------------------------------------------------------------------------------------
// Dense focal classification ("loss_sampling: focal"): no sampling -- every cell of both anchors enters the
// classification term, weighted by alpha_t * (1 - p_t)^gamma, normalised by the number of DISTINCT positive cells N_b = max(1, |P_b|);
// P_b = the cells inside at least one positive window.  The regression rows are those of the sampled modes (every window entry, or the
// centre cell), through reg_entry above.
//
// The grid is (G, B) workgroups over contiguous chunks of the map (hard_chunk: one workgroup for a small map, 35 at cfg2).  One thread
// owns each cell: it reads the four scores and STORES the four gradients, so the classification half has no atomics and does not
// need the zero fill.  A workgroup's partial value goes to its own slot of the workspace; k_focal_fold adds the slots in a fixed
// order in double and rounds once.  Every workgroup stages the sample's windows itself (<= 64 rectangles, <= 1024 entries) and counts
// |P_b| redundantly -- entry (k, cell) is a first occurrence iff no box k' < k holds the cell, <= 4 entries x 64 rectangles per thread --
// which costs less than the launch of a pre-kernel the whole grid would have to wait for.
//
// per-sample workspace, in floats: [0, G) the workgroups' classification partials (not yet divided by N_b), then
constexpr int FS_REG = HARD_MAXG;               // the regression term (without the gain)
constexpr int FS_NPOS = HARD_MAXG + 1;          // |P_b| (an integer below 2^24: exact)
constexpr int FS_STRIDE = HARD_MAXG + 2;

struct LossFocalArgs {
    const float *cls, *reg, *anc, *boxes;
    const int32_t *nbox;
    int64_t cls_bs, reg_bs, gcls_bs, greg_bs;
    float *gcls, *greg, *ws;
    int max_box, box_stride, b0, B, H, W, span, regress_type, reduction, chunk;
    float xs, xo, ys, yo, rs, gain, alpha, gamma, eps;
};

// DCF-DET-BEGIN
// Focal term of one (anchor, cell): adds FL to acc and returns d FL / d p_t, both at q = the clamped probability.  The clamp is a
// comparison, not fmaxf: a NaN score stays NaN and reaches the guarded optimiser step.  The two gradient terms have one sign.
__device__ __forceinline__ float focal_cell(float pt, float alpha_t, float gamma, float eps, float &acc)
{
    const float q = pt < eps ? eps : pt;
    const float lnq = logf(q);
    if (gamma == 0.f) {
        acc += -alpha_t * lnq;
        return -alpha_t / q;
    }
    const float om = 1.f - q;
    const float pw1 = powf(om, gamma - 1.f);    // (1 - q)^(gamma - 1); gamma >= 1, so this is finite at q = 1
    const float pw = pw1 * om;
    acc += -alpha_t * pw * lnq;
    return alpha_t * gamma * pw1 * lnq - alpha_t * pw / q;
}
// DCF-DET-END

template <bool DET>
__global__ void __launch_bounds__(HARD_THREADS) k_loss_focal(LossFocalArgs a)
{
    __shared__ float red[4];
    __shared__ int e_cell[LS_MAXE];            // window entry -> cell, in the reference's order (box, dx, dy): the regression rows
    __shared__ short e_box[LS_MAXE];
    __shared__ int box_first[65], box_cx[64], box_cy[64];
    __shared__ int rx0[64], rx1[64], ry0[64], ry1[64];      // the clipped window of box k; x0 > x1 for a box off the grid
    __shared__ int s_cnt[HARD_THREADS / 64];
    const int g = blockIdx.x, b = a.b0 + blockIdx.y, tid = threadIdx.x;
    const int HW = a.H * a.W, half = a.span / 2;
    const int nb = min(a.nbox[b], a.max_box);
    const float *bx = a.boxes + (int64_t)b * a.max_box * a.box_stride;
    if (tid < nb) {
        // the centre cell exactly as k_loss_sample_fwd_bwd computes it (fp32, one rounding per operation, truncation)
        const int cx = (int)(__fdiv_rn(__fadd_rn(__fmul_rn(bx[tid * a.box_stride], a.xs), a.xo), a.rs));
        const int cy = (int)(__fdiv_rn(__fadd_rn(__fmul_rn(bx[tid * a.box_stride + 1], a.ys), a.yo), a.rs));
        const bool in = !(cx < 0 || cx > a.H - 1 || cy < 0 || cy > a.W - 1);
        box_cx[tid] = in ? cx : -1000000; box_cy[tid] = cy;
        rx0[tid] = in ? max(cx - half, 0) : 0; rx1[tid] = in ? min(cx - half + a.span - 1, a.H - 1) : -1;
        ry0[tid] = in ? max(cy - half, 0) : 0; ry1[tid] = in ? min(cy - half + a.span - 1, a.W - 1) : -1;
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int k = 0; k < nb; ++k) {
            box_first[k] = n;
            n += (rx1[k] - rx0[k] + 1) * (ry1[k] - ry0[k] + 1);      // (0 for a box off the grid)
        }
        box_first[nb > 0 ? nb : 0] = n;
    }
    __syncthreads();
    const int np = min(box_first[nb > 0 ? nb : 0], LS_MAXE);          // (the entry checks max_box * span^2 <= LS_MAXE)
    if (tid < nb) {
        int n = box_first[tid];
        for (int px = rx0[tid]; px <= rx1[tid]; ++px)
            for (int py = ry0[tid]; py <= ry1[tid]; ++py, ++n)
                if (n < LS_MAXE) { e_cell[n] = px * a.W + py; e_box[n] = (short)tid; }
    }
    __syncthreads();
    // ---- |P_b|: the entries whose cell no earlier box holds (integer work: the same count in every workgroup)
    int cnt = 0;
    for (int e = tid; e < np; e += HARD_THREADS) {
        const int cell = e_cell[e], k = e_box[e];
        const int px = cell / a.W, py = cell - px * a.W;
        bool first = true;
        for (int k2 = 0; k2 < k; ++k2) first &= !(px >= rx0[k2] && px <= rx1[k2] && py >= ry0[k2] && py <= ry1[k2]);
        cnt += first ? 1 : 0;
    }
    cnt = wave_sum_i(cnt);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    const int npos = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    const float wsample = sample_weight(a.reduction, a.B);
    const float gscale = (1.f / (float)max(npos, 1)) * wsample;
    // ---- the classification term of this workgroup's cells
    const float *c = a.cls + b * a.cls_bs;
    float *gc = a.gcls + b * a.gcls_bs;
    const int lo = g * a.chunk, hi = min(lo + a.chunk, HW);
    float acc = 0.f;
    // DCF-DET-BEGIN
    for (int cell = lo + tid; cell < hi; cell += HARD_THREADS) {
        const int px = cell / a.W, py = cell - px * a.W;
        bool y = false;
        for (int k = 0; k < nb; ++k) y |= px >= rx0[k] && px <= rx1[k] && py >= ry0[k] && py <= ry1[k];
        const float alpha_t = y ? a.alpha : 1.f - a.alpha;
#pragma unroll
        for (int an = 0; an < 2; ++an) {
            const float s0 = c[(int64_t)(2 * an) * HW + cell], s1 = c[(int64_t)(2 * an + 1) * HW + cell];
            const float gq = focal_cell(y ? s1 : s0, alpha_t, a.gamma, a.eps, acc) * gscale;
            gc[(int64_t)(2 * an) * HW + cell] = y ? 0.f : gq;
            gc[(int64_t)(2 * an + 1) * HW + cell] = y ? gq : 0.f;
        }
    }
    const float part = block_sum<4>(acc, red);
    float *ws = a.ws + (int64_t)b * FS_STRIDE;
    if (tid == 0) ws[g] = part;
    // DCF-DET-END
    if (g != 0) return;
    // ---- the sample's regression rows, in its workgroup 0
    const SampledItems L = {nullptr, nullptr, e_cell, e_box, box_first, box_cx, box_cy, bx, a.box_stride, a.regress_type, a.W, 0, 0, np};
    const SampleMaps m = {c, a.reg + b * a.reg_bs, a.anc, gc, a.greg + b * a.greg_bs, HW, a.gain, wsample};
    float accr = 0.f;
    for (int e = tid; e < np * 14; e += HARD_THREADS) reg_entry<DET>(L, m, e, accr);
    const float regv = block_sum<4>(accr, red);
    if (tid == 0) { ws[FS_REG] = regv; ws[FS_NPOS] = (float)npos; }
}

// loss = sum over the samples that count of wsample * (cls_b + gain * reg_b), cls_b = (partials in workgroup order) / N_b: one thread,
// in double, rounded once; terms [B][3] = (cls_b, reg_b, |P_b|), zero rows for the samples 'last' leaves out
__global__ void k_focal_fold(const float *ws, int B, int b0, int G, float gain, float wsample, float *loss, float *terms)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double tot = 0.0;
    for (int b = 0; b < B; ++b) {
        float *t = terms + 3 * b;
        if (b < b0) { t[0] = 0.f; t[1] = 0.f; t[2] = 0.f; continue; }
        const float *w = ws + (int64_t)b * FS_STRIDE;
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += (double)w[g];
        const double clsv = s / (double)fmaxf(w[FS_NPOS], 1.f);
        t[0] = (float)clsv; t[1] = w[FS_REG]; t[2] = w[FS_NPOS];
        tot += (double)wsample * (clsv + (double)gain * (double)w[FS_REG]);
    }
    *loss = (float)tot;
}

// ---------------------------------------------------------------------------------------------------------------------
// IoU-based anchor assignment ("loss_sampling: anchor"; assign.py is the host statement).  Anchor index
// j = a * HW + cell; I(j, k) = ev_bev_iou(anchor j's rectangle, label k's) in fp64 (ev_geom.h: the evaluation's clip), 0 for a void label
// (a non-finite x, y, l, w or yaw, or l <= 0 or w <= 0).  best(j) = max_k I, arg(j) the lowest k attaining it; forced(k) = the j of highest
// I(j, k) when that is > 0, ties to the lowest j.  target(j) = the lowest k with forced(k) == j, else arg(j) when best >= pos_iou, else -1
// (negative) when best < neg_iou, else -2 (ignored).
//
// A pair whose centres lie further apart than the two half-diagonals together (times AS_PRUNE) skips the clip: the rectangles are
// disjoint and the clip's own value is exactly 0.  Almost every pair goes that way; the 592 B of scratch the clip costs each lane are
// touched by the few lanes near a label.
//   k_assign_force   AS_SEG workgroups per (label, sample), each over a contiguous range of the 2 HW anchors: arg-max through LDS on
//                    (IoU bits, lower j) -- non-negative doubles order like their bit patterns; the partial goes to its own slot
//   k_assign_dense   one thread per cell, both anchors, the sample's labels staged in LDS as fp64 -- and forced(k), folded from the
//                    label's AS_SEG partials in range order; stores target (and best), the workgroup's integer counts go to its own
//                    workspace slot
//   k_assign_fold    adds the slots of a sample, one wave per sample: counts [B][4] = (positives N_b, ignored, positive through forcing only, void labels)
// Integer and fp64 work in a fixed order, no atomics: one entry serves deterministic: true and false.
constexpr int AS_THREADS = 256;
constexpr int AS_SEG = 16;                      // anchor ranges per label in k_assign_force (one workgroup per label left 24 of them
                                                // busy at cfg2: 238 us)
constexpr double AS_PRUNE = 1.002;              // on the squared distance: 0.1 % of slack on the distance, against 1e-16 of rounding

// workspace: the partial arg-max values, u64 [B][max_box][AS_SEG]; their anchors, int [B][max_box][AS_SEG]; the count slots, int [B][G][4]
inline int64_t assign_ws_ints(int B, int HW, int max_box) { return (int64_t)B * max_box * AS_SEG * 3 + (int64_t)B * cdiv(HW, AS_THREADS) * 4; }

struct AssignArgs {
    const float *anc, *boxes;
    const int32_t *nbox;
    int32_t *target, *counts, *part_j, *slots;
    unsigned long long *part_v;
    double *best;
    double pos_iou, neg_iou;
    int max_box, box_stride, B, HW, G;
};

__device__ __forceinline__ bool label_void(const float *bx)
{
    return !(isfinite(bx[0]) && isfinite(bx[1]) && isfinite(bx[3]) && isfinite(bx[4]) && isfinite(bx[6]) && bx[3] > 0.f && bx[4] > 0.f);
}
__device__ __forceinline__ double half_diag(double l, double w) { return 0.5 * sqrt(l * l + w * w); }
// the seven parameters of anchor (a, cell), gathered from [2][7][HW]
__device__ __forceinline__ void anchor_row(const float *anc, int a, int cell, int HW, float (&row)[7])
{
#pragma unroll
    for (int c = 0; c < 7; ++c) row[c] = anc[((int64_t)a * 7 + c) * HW + cell];
}

__global__ void __launch_bounds__(AS_THREADS) k_assign_force(AssignArgs a)
{
    __shared__ unsigned long long s_val[AS_THREADS];
    __shared__ int s_j[AS_THREADS];
    const int k = blockIdx.x, b = blockIdx.y, seg = blockIdx.z, tid = threadIdx.x;
    const int nb = max(min(a.nbox[b], a.max_box), 0);
    const int64_t slot = ((int64_t)b * a.max_box + k) * AS_SEG + seg;
    const float *bx = a.boxes + ((int64_t)b * a.max_box + k) * a.box_stride;
    if (k >= nb || label_void(bx)) {               // (uniform over the workgroup)
        if (tid == 0) { a.part_v[slot] = 0ull; a.part_j[slot] = -1; }
        return;
    }
    const int per = (int)(((int64_t)2 * a.HW + AS_SEG - 1) / AS_SEG), lo = seg * per, hi = lo + max(min(per, 2 * a.HW - lo), 0);
    double lab[4][2];
    ev_rect(bx, lab);
    const double lx = bx[0], ly = bx[1], lh = half_diag(bx[3], bx[4]);
    unsigned long long bv = 0ull;                   // bits of the best IoU so far (+0.0), and its anchor
    int bj = -1;
    for (int j = lo + tid; j < hi; j += AS_THREADS) {
        const int an = j >= a.HW ? 1 : 0, cell = j - an * a.HW;
        float row[7];
        anchor_row(a.anc, an, cell, a.HW, row);
        const double dx = (double)row[0] - lx, dy = (double)row[1] - ly, s = half_diag(row[3], row[4]) + lh;
        if (dx * dx + dy * dy > s * s * AS_PRUNE) continue;
        double rect[4][2];
        ev_rect(row, rect);
        const unsigned long long v = (unsigned long long)__double_as_longlong(ev_bev_iou(rect, lab));
        if (v > bv && v <= 0x7ff0000000000000ull) { bv = v; bj = j; }      // (j ascends: the first of equal values stays)
    }
    s_val[tid] = bv; s_j[tid] = bj;
    __syncthreads();
    for (int o = AS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const unsigned long long v2 = s_val[tid + o];
            const int j2 = s_j[tid + o];
            if (v2 > s_val[tid] || (v2 == s_val[tid] && v2 != 0ull && j2 < s_j[tid])) { s_val[tid] = v2; s_j[tid] = j2; }
        }
        __syncthreads();
    }
    if (tid == 0) { a.part_v[slot] = s_val[0]; a.part_j[slot] = s_val[0] != 0ull ? s_j[0] : -1; }
}

__global__ void __launch_bounds__(AS_THREADS) k_assign_dense(AssignArgs a)
{
    __shared__ double l_rect[64][4][2];
    __shared__ double l_x[64], l_y[64], l_h[64];
    __shared__ int l_ok[64], l_forced[64];
    __shared__ int s_cnt[AS_THREADS / 64][3];
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nb = max(min(a.nbox[b], a.max_box), 0);           // (the entry checks max_box <= 64)
    if (tid < nb) {
        const float *bx = a.boxes + ((int64_t)b * a.max_box + tid) * a.box_stride;
        const bool ok = !label_void(bx);
        l_ok[tid] = ok ? 1 : 0;
        unsigned long long fv = 0ull;                               // forced(tid): the ranges ascend in j, so the first of equal values stays
        int fj = -1;
        for (int q = 0; q < AS_SEG; ++q) {
            const int64_t slot = ((int64_t)b * a.max_box + tid) * AS_SEG + q;
            if (a.part_v[slot] > fv) { fv = a.part_v[slot]; fj = a.part_j[slot]; }
        }
        l_forced[tid] = fj;
        if (ok) {
            ev_rect(bx, l_rect[tid]);
            l_x[tid] = bx[0]; l_y[tid] = bx[1]; l_h[tid] = half_diag(bx[3], bx[4]);
        }
    }
    __syncthreads();
    const int cell = g * AS_THREADS + tid;
    int npos = 0, nign = 0, nforced = 0;
    if (cell < a.HW) {
#pragma unroll 1
        for (int an = 0; an < 2; ++an) {
            const int j = an * a.HW + cell;
            float row[7];
            anchor_row(a.anc, an, cell, a.HW, row);
            const double ax = row[0], ay = row[1], ah = half_diag(row[3], row[4]);
            double rect[4][2];
            bool have = false;
            double best = 0.0;
            int arg = nb > 0 ? 0 : -1;
            for (int k = 0; k < nb; ++k) {
                if (!l_ok[k]) continue;
                const double dx = ax - l_x[k], dy = ay - l_y[k], s = ah + l_h[k];
                if (dx * dx + dy * dy > s * s * AS_PRUNE) continue;
                if (!have) { ev_rect(row, rect); have = true; }
                const double v = ev_bev_iou(rect, l_rect[k]);
                if (v > best) { best = v; arg = k; }
            }
            int t = -3;
            for (int k = nb - 1; k >= 0; --k) t = l_forced[k] == j ? k : t;      // the lowest k that forces j
            if (t >= 0) {
                nforced += best >= a.pos_iou ? 0 : 1;
            } else if (best >= a.pos_iou) {
                t = arg;
            } else {
                t = best < a.neg_iou ? -1 : -2;
            }
            npos += t >= 0 ? 1 : 0;
            nign += t == -2 ? 1 : 0;
            a.target[(int64_t)b * 2 * a.HW + j] = t;
            if (a.best) a.best[(int64_t)b * 2 * a.HW + j] = best;
        }
    }
    npos = wave_sum_i(npos); nign = wave_sum_i(nign); nforced = wave_sum_i(nforced);
    if ((tid & 63) == 0) { s_cnt[tid >> 6][0] = npos; s_cnt[tid >> 6][1] = nign; s_cnt[tid >> 6][2] = nforced; }
    __syncthreads();
    if (tid == 0) {
        int32_t *slot = a.slots + ((int64_t)b * a.G + g) * 4;
        int nvoid = 0;
        for (int k = 0; k < nb; ++k) nvoid += l_ok[k] ? 0 : 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) slot[c] = (s_cnt[0][c] + s_cnt[1][c]) + (s_cnt[2][c] + s_cnt[3][c]);
        slot[3] = g == 0 ? nvoid : 0;
    }
}

// one wave per sample (integer sums: any order gives the same counts)
__global__ void __launch_bounds__(64) k_assign_fold(const int32_t *slots, int G, int32_t *counts)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    int c[4] = {0, 0, 0, 0};
    for (int g = lane; g < G; g += 64)
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] += slots[((int64_t)b * G + g) * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] = wave_sum_i(c[q]);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < 4; ++q) counts[4 * b + q] = c[q];
}

// The terms on per-anchor targets: the shape of k_loss_focal -- (G, B) workgroups over contiguous chunks, one thread per cell.  Every
// cell of a computed sample gets all 4 classification and all 14 regression gradients STORED (zeros where a term is absent): no
// atomics, no dependence on a zero fill.  A target outside [-2, max_box) counts as ignored.  N_b = counts[b][0].
// per-sample workspace, in floats: [0, G) the classification partials, [HARD_MAXG, HARD_MAXG + G) the regression partials (both
// undivided)
constexpr int AL_STRIDE = 2 * HARD_MAXG;

struct LossAnchorArgs {
    const float *cls, *reg, *anc, *boxes;
    const int32_t *target, *counts;
    int64_t cls_bs, reg_bs, gcls_bs, greg_bs;
    float *gcls, *greg, *ws;
    int max_box, box_stride, b0, B, HW, reduction, chunk;
    float gain, alpha, gamma, eps;
};

__global__ void __launch_bounds__(HARD_THREADS) k_loss_anchor(LossAnchorArgs a)
{
    __shared__ float red[4];
    const int g = blockIdx.x, b = a.b0 + blockIdx.y, tid = threadIdx.x;
    const int HW = a.HW;
    const int npos = max(a.counts[4 * b], 1);
    const float wsample = sample_weight(a.reduction, a.B);
    const float gscale = (1.f / (float)npos) * wsample;
    const float rscale = a.gain * wsample / (7.f * (float)npos);
    const float *c = a.cls + b * a.cls_bs, *r = a.reg + b * a.reg_bs;
    const float *bx = a.boxes + (int64_t)b * a.max_box * a.box_stride;
    const int32_t *tg = a.target + (int64_t)b * 2 * HW;
    float *gc = a.gcls + b * a.gcls_bs, *gr = a.greg + b * a.greg_bs;
    const int lo = g * a.chunk, hi = min(lo + a.chunk, HW);
    float acc = 0.f, accr = 0.f;
    for (int cell = lo + tid; cell < hi; cell += HARD_THREADS) {
#pragma unroll
        for (int an = 0; an < 2; ++an) {
            int t = tg[(int64_t)an * HW + cell];
            if (t < -2 || t >= a.max_box) t = -2;
            const bool y = t >= 0;
            const float s0 = c[(int64_t)(2 * an) * HW + cell], s1 = c[(int64_t)(2 * an + 1) * HW + cell];
            float g0 = 0.f, g1 = 0.f;
            if (t != -2) {
                const float gq = focal_cell(y ? s1 : s0, y ? a.alpha : 1.f - a.alpha, a.gamma, a.eps, acc) * gscale;
                g0 = y ? 0.f : gq; g1 = y ? gq : 0.f;
            }
            gc[(int64_t)(2 * an) * HW + cell] = g0;
            gc[(int64_t)(2 * an + 1) * HW + cell] = g1;
            const float *anp = a.anc + (int64_t)an * 7 * HW + cell;
            const float *box = bx + (int64_t)(y ? t : 0) * a.box_stride;
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                float gv = 0.f;
                if (y) {
                    const float d = r[(int64_t)(7 * an + q) * HW + cell] - reg_target(box, anp, q, HW);
                    const float ad = fabsf(d);
                    accr += ad < 1.f ? 0.5f * d * d : ad - 0.5f;
                    gv = sl1_grad(d) * rscale;
                }
                gr[(int64_t)(7 * an + q) * HW + cell] = gv;
            }
        }
    }
    float *ws = a.ws + (int64_t)b * AL_STRIDE;
    const float part = block_sum<4>(acc, red);
    const float partr = block_sum<4>(accr, red);
    if (tid == 0) { ws[g] = part; ws[HARD_MAXG + g] = partr; }
}

// loss = sum over the samples that count of wsample * (cls_b + gain * reg_b): one thread, the partials in workgroup order in double,
// rounded once; terms [B][3] = (cls_b, reg_b, N_b), zero rows for the samples 'last' leaves out
__global__ void k_anchor_fold(const float *ws, const int32_t *counts, int B, int b0, int G, float gain, float wsample, float *loss, float *terms)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double tot = 0.0;
    for (int b = 0; b < B; ++b) {
        float *t = terms + 3 * b;
        if (b < b0) { t[0] = 0.f; t[1] = 0.f; t[2] = 0.f; continue; }
        const float *w = ws + (int64_t)b * AL_STRIDE;
        double s = 0.0, sr = 0.0;
        for (int g = 0; g < G; ++g) { s += (double)w[g]; sr += (double)w[HARD_MAXG + g]; }
        const int n = counts[4 * b];
        const double den = (double)max(n, 1);
        const double clsv = s / den, regv = sr / (7.0 * den);
        t[0] = (float)clsv; t[1] = (float)regv; t[2] = (float)n;
        tot += (double)wsample * (clsv + (double)gain * regv);
    }
    *loss = (float)tot;
}

}  // namespace

extern "C" uint32_t dcf_loss_sample_rand(uint64_t seed, int sample, int stream, int index, int attempt)
{
    return dcf_loss_rand(seed, sample, stream, index, attempt);
}

static int loss_sample_impl(const char *who, bool hard, void *hard_ws, float *loss_rows, const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                                       const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                                       float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, int pos_cap,
                                       int neg_count, uint64_t seed, float reg_gain, int reduction, float *loss, float *gcls,
                                       int64_t gcls_bstride, float *greg, int64_t greg_bstride, int32_t *pos_out, int32_t *neg_out,
                                       int32_t *counts_out, dcf_stream_t stream)
{
    DCF_REQUIRE(cls && reg && anchors && boxes && nbox_dev && loss && gcls && greg && B > 0 && H > 0 && W > 0, "%s: bad arguments", who);
    DCF_REQUIRE(reduction >= 0 && reduction <= 2, "%s: reduction must be 0 (last), 1 (sum) or 2 (mean)", who);
    DCF_REQUIRE(max_box >= 0 && max_box <= 64 && span >= 1 && max_box * span * span <= LS_MAXE && box_stride >= 7,
                "%s: at most 64 boxes and %d window cells per sample", who, LS_MAXE);
    DCF_REQUIRE(pos_cap >= 1 && pos_cap <= LS_MAXE && neg_count >= 1 && neg_count <= LS_MAXNEG, "%s: pos_cap <= %d, neg_count <= %d", who, LS_MAXE, LS_MAXNEG);
    LossSampleArgs a;
    a.loss_rows = loss_rows;
    a.cls = cls; a.reg = reg; a.anc = anchors; a.boxes = boxes; a.nbox = nbox_dev;
    a.cls_bs = cls_bstride; a.reg_bs = reg_bstride; a.gcls_bs = gcls_bstride; a.greg_bs = greg_bstride;
    a.loss = loss; a.gcls = gcls; a.greg = greg; a.pos_out = pos_out; a.neg_out = neg_out; a.counts_out = counts_out;
    a.seed = seed; a.max_box = max_box; a.box_stride = box_stride; a.B = B; a.H = H; a.W = W; a.span = span;
    a.regress_type = regress_type; a.pos_cap = pos_cap; a.neg_count = neg_count; a.reduction = reduction;
    a.xs = xs; a.xo = xo; a.ys = ys; a.yo = yo; a.rs = reduced_scale; a.gain = reg_gain;
    a.hard_ws = nullptr; a.hard_stride = 0; a.hard_b0 = 0;
    hipStream_t s = S(stream);
    if (hard) {
        DCF_REQUIRE(hard_ws && ((uintptr_t)hard_ws & 3) == 0, "%s: null or misaligned workspace", who);
        DCF_REQUIRE((int64_t)H * W < (int64_t)1 << 30, "%s: map too large", who);
        const int HW = H * W;
        HardArgs h;
        h.cls = cls; h.boxes = boxes; h.nbox = nbox_dev; h.cls_bs = cls_bstride; h.ws_stride = hard_ws_stride(HW); h.ws = (int32_t *)hard_ws;
        h.max_box = max_box; h.box_stride = box_stride; h.H = H; h.W = W; h.span = span; h.neg_count = neg_count;
        h.xs = xs; h.xo = xo; h.ys = ys; h.yo = yo; h.rs = reduced_scale;
        h.chunk = hard_chunk(HW);
        h.G = cdiv(HW, h.chunk);
        // 'last' with no lists asked for: only the last sample's negatives are ever read
        h.b0 = (reduction == 0 && !neg_out && !counts_out) ? B - 1 : 0;
        a.hard_ws = h.ws; a.hard_stride = h.ws_stride; a.hard_b0 = h.b0;
        const dim3 grid(h.G, B - h.b0);
        const double map_bytes = (double)(B - h.b0) * HW * 4.0;
        DCF_LAUNCH_B("loss_hard_keys", 5.0 * map_bytes, s, hipLaunchKernelGGL(k_hard_keys, grid, dim3(HARD_THREADS), 0, s, h));
        for (int p = 1; p <= 3; ++p)
            DCF_LAUNCH_B("loss_hard_pass", map_bytes, s, hipLaunchKernelGGL(k_hard_pass, grid, dim3(HARD_THREADS), 0, s, h, p));
        DCF_LAUNCH_B("loss_hard_compact", map_bytes, s, hipLaunchKernelGGL(k_hard_compact, grid, dim3(HARD_THREADS), 0, s, h));
        if (loss_rows) {
            DCF_LAUNCH("loss_hard_fwd_bwd_det", s, hipLaunchKernelGGL((k_loss_sample_fwd_bwd<true, true>), dim3(B), dim3(256), 0, s, a));
            DCF_LAUNCH("loss_rows_fold", s, hipLaunchKernelGGL(k_loss_rows_fold, dim3(1), dim3(64), 0, s, loss_rows, B, loss));
        } else {
            DCF_LAUNCH("loss_hard_fwd_bwd", s, hipLaunchKernelGGL((k_loss_sample_fwd_bwd<false, true>), dim3(B), dim3(256), 0, s, a));
        }
        return DCF_OK;
    }
    if (loss_rows) {
        DCF_LAUNCH("loss_sample_fwd_bwd_det", s, hipLaunchKernelGGL(k_loss_sample_fwd_bwd<true>, dim3(B), dim3(256), 0, s, a));
        DCF_LAUNCH("loss_rows_fold", s, hipLaunchKernelGGL(k_loss_rows_fold, dim3(1), dim3(64), 0, s, loss_rows, B, loss));
    } else {
        DCF_LAUNCH("loss_sample_fwd_bwd", s, hipLaunchKernelGGL(k_loss_sample_fwd_bwd<false>, dim3(B), dim3(256), 0, s, a));
    }
    return DCF_OK;
}

extern "C" int dcf_loss_sample_fwd_bwd(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                                       const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                                       float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, int pos_cap,
                                       int neg_count, uint64_t seed, float reg_gain, int reduction, float *loss, float *gcls,
                                       int64_t gcls_bstride, float *greg, int64_t greg_bstride, int32_t *pos_out, int32_t *neg_out,
                                       int32_t *counts_out, dcf_stream_t stream)
{
    return loss_sample_impl("dcf_loss_sample_fwd_bwd", false, nullptr, nullptr, cls, cls_bstride, reg, reg_bstride, anchors, boxes, nbox_dev, max_box, box_stride, B, H, W, xs,
                            xo, ys, yo, reduced_scale, span, regress_type, pos_cap, neg_count, seed, reg_gain, reduction, loss, gcls, gcls_bstride, greg,
                            greg_bstride, pos_out, neg_out, counts_out, stream);
}

// The same launch in one fixed summation order (deterministic: true); loss_rows: B floats of scratch.
extern "C" int dcf_loss_sample_fwd_bwd_det(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                                           const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                                           float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, int pos_cap,
                                           int neg_count, uint64_t seed, float reg_gain, int reduction, float *loss, float *gcls,
                                           int64_t gcls_bstride, float *greg, int64_t greg_bstride, int32_t *pos_out, int32_t *neg_out,
                                           int32_t *counts_out, float *loss_rows, dcf_stream_t stream)
{
    DCF_REQUIRE(loss_rows, "dcf_loss_sample_fwd_bwd_det: null loss_rows");
    return loss_sample_impl("dcf_loss_sample_fwd_bwd_det", false, nullptr, loss_rows, cls, cls_bstride, reg, reg_bstride, anchors, boxes, nbox_dev, max_box, box_stride, B, H,
                            W, xs, xo, ys, yo, reduced_scale, span, regress_type, pos_cap, neg_count, seed, reg_gain, reduction, loss, gcls, gcls_bstride,
                            greg, greg_bstride, pos_out, neg_out, counts_out, stream);
}

// loss_sampling: hard (the selection kernels above, then the device mode's positives and terms)
extern "C" size_t dcf_loss_hard_workspace_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W >= (int64_t)1 << 30) return 0;
    return (size_t)B * (size_t)hard_ws_stride(H * W) * sizeof(int32_t);
}

extern "C" int dcf_loss_hard_fwd_bwd(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                                     const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                                     float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, int pos_cap,
                                     int neg_count, uint64_t seed, float reg_gain, int reduction, float *loss, float *gcls,
                                     int64_t gcls_bstride, float *greg, int64_t greg_bstride, int32_t *pos_out, int32_t *neg_out,
                                     int32_t *counts_out, void *workspace, dcf_stream_t stream)
{
    return loss_sample_impl("dcf_loss_hard_fwd_bwd", true, workspace, nullptr, cls, cls_bstride, reg, reg_bstride, anchors, boxes, nbox_dev, max_box,
                            box_stride, B, H, W, xs, xo, ys, yo, reduced_scale, span, regress_type, pos_cap, neg_count, seed, reg_gain, reduction, loss,
                            gcls, gcls_bstride, greg, greg_bstride, pos_out, neg_out, counts_out, stream);
}

extern "C" int dcf_loss_hard_fwd_bwd_det(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                                         const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                                         float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, int pos_cap,
                                         int neg_count, uint64_t seed, float reg_gain, int reduction, float *loss, float *gcls,
                                         int64_t gcls_bstride, float *greg, int64_t greg_bstride, int32_t *pos_out, int32_t *neg_out,
                                         int32_t *counts_out, void *workspace, float *loss_rows, dcf_stream_t stream)
{
    DCF_REQUIRE(loss_rows, "dcf_loss_hard_fwd_bwd_det: null loss_rows");
    return loss_sample_impl("dcf_loss_hard_fwd_bwd_det", true, workspace, loss_rows, cls, cls_bstride, reg, reg_bstride, anchors, boxes, nbox_dev, max_box,
                            box_stride, B, H, W, xs, xo, ys, yo, reduced_scale, span, regress_type, pos_cap, neg_count, seed, reg_gain, reduction, loss,
                            gcls, gcls_bstride, greg, greg_bstride, pos_out, neg_out, counts_out, stream);
}

// loss_sampling: focal (k_loss_focal over the whole map, then the fold)
extern "C" size_t dcf_loss_focal_workspace_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W >= (int64_t)1 << 30) return 0;
    return (size_t)B * FS_STRIDE * sizeof(float);
}

static int loss_focal_impl(const char *who, bool det, const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                           const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W, float xs, float xo,
                           float ys, float yo, float reduced_scale, int span, int regress_type, float alpha, float gamma, float eps,
                           float reg_gain, int reduction, float *loss, float *gcls, int64_t gcls_bstride, float *greg, int64_t greg_bstride,
                           float *terms, void *workspace, dcf_stream_t stream)
{
    DCF_REQUIRE(cls && reg && anchors && boxes && nbox_dev && loss && gcls && greg && terms && B > 0 && H > 0 && W > 0, "%s: bad arguments", who);
    DCF_REQUIRE(reduction >= 0 && reduction <= 2, "%s: reduction must be 0 (last), 1 (sum) or 2 (mean)", who);
    DCF_REQUIRE(max_box >= 0 && max_box <= 64 && span >= 1 && max_box * span * span <= LS_MAXE && box_stride >= 7,
                "%s: at most 64 boxes and %d window cells per sample", who, LS_MAXE);
    DCF_REQUIRE((int64_t)H * W < (int64_t)1 << 30, "%s: map too large", who);
    DCF_REQUIRE(alpha > 0.f && alpha < 1.f && (gamma == 0.f || gamma >= 1.f) && eps > 0.f && eps <= 1e-3f,
                "%s: alpha in (0, 1), gamma 0 or >= 1, eps in (0, 1e-3]", who);
    DCF_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0, "%s: null or misaligned workspace", who);
    const int HW = H * W;
    LossFocalArgs a;
    a.cls = cls; a.reg = reg; a.anc = anchors; a.boxes = boxes; a.nbox = nbox_dev;
    a.cls_bs = cls_bstride; a.reg_bs = reg_bstride; a.gcls_bs = gcls_bstride; a.greg_bs = greg_bstride;
    a.gcls = gcls; a.greg = greg; a.ws = (float *)workspace;
    a.max_box = max_box; a.box_stride = box_stride; a.B = B; a.H = H; a.W = W; a.span = span; a.regress_type = regress_type;
    a.reduction = reduction; a.chunk = hard_chunk(HW);
    a.b0 = reduction == 0 ? B - 1 : 0;              // 'last': only the last sample is computed
    a.xs = xs; a.xo = xo; a.ys = ys; a.yo = yo; a.rs = reduced_scale; a.gain = reg_gain; a.alpha = alpha; a.gamma = gamma; a.eps = eps;
    const int G = cdiv(HW, a.chunk);
    const dim3 grid(G, B - a.b0);
    const double map_bytes = (double)(B - a.b0) * HW * 4.0;
    hipStream_t s = S(stream);
    if (det)
        DCF_LAUNCH_B("loss_focal_fwd_bwd_det", 8.0 * map_bytes, s, hipLaunchKernelGGL(k_loss_focal<true>, grid, dim3(HARD_THREADS), 0, s, a));
    else
        DCF_LAUNCH_B("loss_focal_fwd_bwd", 8.0 * map_bytes, s, hipLaunchKernelGGL(k_loss_focal<false>, grid, dim3(HARD_THREADS), 0, s, a));
    DCF_LAUNCH("loss_focal_fold", s, hipLaunchKernelGGL(k_focal_fold, dim3(1), dim3(64), 0, s, a.ws, B, a.b0, G, reg_gain, sample_weight(reduction, B), loss, terms));
    return DCF_OK;
}

extern "C" int dcf_loss_focal_fwd_bwd(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                                      const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                                      float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, float alpha,
                                      float gamma, float eps, float reg_gain, int reduction, float *loss, float *gcls, int64_t gcls_bstride,
                                      float *greg, int64_t greg_bstride, float *terms, void *workspace, dcf_stream_t stream)
{
    return loss_focal_impl("dcf_loss_focal_fwd_bwd", false, cls, cls_bstride, reg, reg_bstride, anchors, boxes, nbox_dev, max_box, box_stride, B, H, W, xs,
                           xo, ys, yo, reduced_scale, span, regress_type, alpha, gamma, eps, reg_gain, reduction, loss, gcls, gcls_bstride, greg,
                           greg_bstride, terms, workspace, stream);
}

// The same launch with the regression gradients summed in one fixed order (deterministic: true); everything else is already fixed.
extern "C" int dcf_loss_focal_fwd_bwd_det(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                                          const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H, int W,
                                          float xs, float xo, float ys, float yo, float reduced_scale, int span, int regress_type, float alpha,
                                          float gamma, float eps, float reg_gain, int reduction, float *loss, float *gcls, int64_t gcls_bstride,
                                          float *greg, int64_t greg_bstride, float *terms, void *workspace, dcf_stream_t stream)
{
    return loss_focal_impl("dcf_loss_focal_fwd_bwd_det", true, cls, cls_bstride, reg, reg_bstride, anchors, boxes, nbox_dev, max_box, box_stride, B, H, W,
                           xs, xo, ys, yo, reduced_scale, span, regress_type, alpha, gamma, eps, reg_gain, reduction, loss, gcls, gcls_bstride, greg,
                           greg_bstride, terms, workspace, stream);
}

extern "C" int dcf_loss_fwd_bwd_det(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                                    const int64_t *ints, const float *floats, int B, int HW, float reg_gain, int reduction, float *loss,
                                    float *gcls, int64_t gcls_bstride, float *greg, int64_t greg_bstride, float *loss_rows, dcf_stream_t stream)
{
    DCF_REQUIRE(cls && reg && anchors && ints && floats && loss && gcls && greg && loss_rows && B > 0 && HW > 0, "dcf_loss_fwd_bwd_det: bad arguments");
    DCF_REQUIRE(reduction >= 0 && reduction <= 2, "dcf_loss_fwd_bwd_det: reduction must be 0 (last), 1 (sum) or 2 (mean)");
    hipStream_t s = S(stream);
    DCF_LAUNCH("loss_fwd_bwd_det", s, hipLaunchKernelGGL(k_loss_fwd_bwd<true>, dim3(B), dim3(1024), 0, s, cls, cls_bstride, reg, reg_bstride, anchors, ints,
                                                         floats, B, HW, reg_gain, reduction, loss, gcls, gcls_bstride, greg, greg_bstride, loss_rows));
    DCF_LAUNCH("loss_rows_fold", s, hipLaunchKernelGGL(k_loss_rows_fold, dim3(1), dim3(64), 0, s, loss_rows, B, loss));
    return DCF_OK;
}

extern "C" int dcf_loss_fwd_bwd(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                                const int64_t *ints, const float *floats, int B, int HW, float reg_gain, int reduction,
                                float *loss, float *gcls, int64_t gcls_bstride, float *greg, int64_t greg_bstride, dcf_stream_t stream)
{
    DCF_REQUIRE(cls && reg && anchors && ints && floats && loss && gcls && greg && B > 0 && HW > 0, "dcf_loss_fwd_bwd: bad arguments");
    DCF_REQUIRE(reduction >= 0 && reduction <= 2, "dcf_loss_fwd_bwd: reduction must be 0 (last), 1 (sum) or 2 (mean)");
    hipStream_t s = S(stream);
    DCF_LAUNCH("loss_fwd_bwd", s, hipLaunchKernelGGL(k_loss_fwd_bwd<false>, dim3(B), dim3(1024), 0, s, cls, cls_bstride, reg, reg_bstride, anchors, ints,
                                                     floats, B, HW, reg_gain, reduction, loss, gcls, gcls_bstride, greg, greg_bstride, (float *)nullptr));
    return DCF_OK;
}

// loss_sampling: anchor -- the assignment (k_assign_force, k_assign_dense, k_assign_fold) ...
extern "C" size_t dcf_assign_anchors_workspace_bytes(int B, int H, int W, int max_box)
{
    if (B <= 0 || H <= 0 || W <= 0 || max_box < 1 || max_box > 64 || (int64_t)H * W >= (int64_t)1 << 30) return 0;
    return (size_t)assign_ws_ints(B, H * W, max_box) * sizeof(int32_t);
}

extern "C" int dcf_assign_anchors_iou(const float *anchors, const float *boxes, const int32_t *nbox_dev, int max_box, int box_stride, int B, int H,
                                      int W, double pos_iou, double neg_iou, int32_t *target, double *best, int32_t *counts, void *workspace,
                                      dcf_stream_t stream)
{
    DCF_REQUIRE(anchors && boxes && nbox_dev && target && counts && B > 0 && H > 0 && W > 0, "dcf_assign_anchors_iou: bad arguments");
    DCF_REQUIRE(max_box >= 1 && max_box <= 64 && box_stride >= 7, "dcf_assign_anchors_iou: 1 to 64 boxes per sample, at least 7 values each");
    DCF_REQUIRE((int64_t)H * W < (int64_t)1 << 30, "dcf_assign_anchors_iou: map too large");
    DCF_REQUIRE(neg_iou > 0.0 && neg_iou <= pos_iou && pos_iou <= 1.0, "dcf_assign_anchors_iou: 0 < neg_iou <= pos_iou <= 1");
    DCF_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && (!best || ((uintptr_t)best & 7) == 0), "dcf_assign_anchors_iou: null or misaligned workspace / best");
    AssignArgs a;
    a.anc = anchors; a.boxes = boxes; a.nbox = nbox_dev; a.target = target; a.best = best; a.counts = counts;
    a.part_v = (unsigned long long *)workspace; a.part_j = (int32_t *)(a.part_v + (int64_t)B * max_box * AS_SEG);
    a.slots = a.part_j + (int64_t)B * max_box * AS_SEG;
    a.pos_iou = pos_iou; a.neg_iou = neg_iou; a.max_box = max_box; a.box_stride = box_stride; a.B = B; a.HW = H * W;
    a.G = cdiv(a.HW, AS_THREADS);
    hipStream_t s = S(stream);
    DCF_LAUNCH("assign_force", s, hipLaunchKernelGGL(k_assign_force, dim3(max_box, B, AS_SEG), dim3(AS_THREADS), 0, s, a));
    DCF_LAUNCH_B("assign_dense", (double)B * a.HW * (14.0 * 4 + 2 * 4 + (best ? 16.0 : 0.0)), s,
                 hipLaunchKernelGGL(k_assign_dense, dim3(a.G, B), dim3(AS_THREADS), 0, s, a));
    DCF_LAUNCH("assign_fold", s, hipLaunchKernelGGL(k_assign_fold, dim3(B), dim3(64), 0, s, a.slots, a.G, counts));
    return DCF_OK;
}

// ... and the terms on its targets (k_loss_anchor over the whole map, then the fold)
extern "C" size_t dcf_loss_anchor_workspace_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W >= (int64_t)1 << 30) return 0;
    return (size_t)B * AL_STRIDE * sizeof(float);
}

extern "C" int dcf_loss_anchor_fwd_bwd(const float *cls, int64_t cls_bstride, const float *reg, int64_t reg_bstride, const float *anchors,
                                       const float *boxes, int max_box, int box_stride, const int32_t *target, const int32_t *counts, int B, int H,
                                       int W, float alpha, float gamma, float eps, float reg_gain, int reduction, float *loss, float *gcls,
                                       int64_t gcls_bstride, float *greg, int64_t greg_bstride, float *terms, void *workspace, dcf_stream_t stream)
{
    DCF_REQUIRE(cls && reg && anchors && boxes && target && counts && loss && gcls && greg && terms && B > 0 && H > 0 && W > 0,
                "dcf_loss_anchor_fwd_bwd: bad arguments");
    DCF_REQUIRE(reduction >= 0 && reduction <= 2, "dcf_loss_anchor_fwd_bwd: reduction must be 0 (last), 1 (sum) or 2 (mean)");
    DCF_REQUIRE(max_box >= 1 && max_box <= 64 && box_stride >= 7, "dcf_loss_anchor_fwd_bwd: 1 to 64 boxes per sample, at least 7 values each");
    DCF_REQUIRE((int64_t)H * W < (int64_t)1 << 30, "dcf_loss_anchor_fwd_bwd: map too large");
    DCF_REQUIRE(alpha > 0.f && alpha < 1.f && (gamma == 0.f || gamma >= 1.f) && eps > 0.f && eps <= 1e-3f,
                "dcf_loss_anchor_fwd_bwd: alpha in (0, 1), gamma 0 or >= 1, eps in (0, 1e-3]");
    DCF_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0, "dcf_loss_anchor_fwd_bwd: null or misaligned workspace");
    const int HW = H * W;
    LossAnchorArgs a;
    a.cls = cls; a.reg = reg; a.anc = anchors; a.boxes = boxes; a.target = target; a.counts = counts;
    a.cls_bs = cls_bstride; a.reg_bs = reg_bstride; a.gcls_bs = gcls_bstride; a.greg_bs = greg_bstride;
    a.gcls = gcls; a.greg = greg; a.ws = (float *)workspace;
    a.max_box = max_box; a.box_stride = box_stride; a.B = B; a.HW = HW; a.reduction = reduction; a.chunk = hard_chunk(HW);
    a.b0 = reduction == 0 ? B - 1 : 0;              // 'last': only the last sample is computed
    a.gain = reg_gain; a.alpha = alpha; a.gamma = gamma; a.eps = eps;
    const int G = cdiv(HW, a.chunk);
    hipStream_t s = S(stream);
    DCF_LAUNCH_B("loss_anchor_fwd_bwd", (double)(B - a.b0) * HW * 4.0 * 38.0, s,
                 hipLaunchKernelGGL(k_loss_anchor, dim3(G, B - a.b0), dim3(HARD_THREADS), 0, s, a));
    DCF_LAUNCH("loss_anchor_fold", s, hipLaunchKernelGGL(k_anchor_fold, dim3(1), dim3(64), 0, s, a.ws, counts, B, a.b0, G, reg_gain,
                                                          sample_weight(reduction, B), loss, terms));
    return DCF_OK;
}
