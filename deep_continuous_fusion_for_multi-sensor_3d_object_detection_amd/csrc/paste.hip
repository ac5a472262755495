// paste.hip -- train-time object pasting (host statements and sampler: paste.py, bank: objbank.py).
//
// Two launches per step, both over the frames of a batch (blockIdx.y = frame):
//   k_paste_points_b   rows of the scene inside a pasted box become +inf rows (the convention of the point drop: every range test
//                      rejects them), the bank's rows of the pasted objects are appended behind the scene's
//   k_paste_patches_b  the pasted objects' image patches are painted into a copy of the image, a pure function of the output pixel
// The per-frame tables (16 records each) are 5 KB for 8 frames -- over the 4 KB a kernel takes by value.  Up to four frames (the
// cfg2 batch has two) they travel in the kernel argument; five to eight travel as ONE asynchronous copy on the launch's own stream
// out of a pinned buffer the caller owns (a ring slot, ops.py), which costs about as much again as the launch.  Either way the
// kernels read them with wave-uniform loads, and the host validates every index first: the kernels trust the table.
//
// Bit-exactness contract (points): every product, sum and difference of the inside test is spelled __fmul_rn / __fadd_rn /
// __fsub_rn (and the file is built with -ffp-contract=off like the rest of the library), so each rounds where paste.inside_mask's
// np.float32 arithmetic rounds.  Rows are moved as dwords: a NaN keeps its payload.
#include <limits.h>

#include "dcf_common.h"

namespace {

constexpr int PST_BATCH_MAX = 8;       // frames per launch (DCF_PROJ_BATCH_MAX of geometry.hip)
constexpr int PST_REC_MAX = 16;        // records per frame
constexpr int PST_THREADS = 256;
constexpr int PST_ITEMS = 4;
constexpr int PST_TILE = PST_THREADS * PST_ITEMS;

struct PstPointsFrame {
    const unsigned *pts;
    unsigned *out;
    int n, m, a, pad;
    float rec[PST_REC_MAX][8];         // cx cy cz c s hl hw hh
    int start[PST_REC_MAX];            // first bank row of object j
    int pre[PST_REC_MAX + 1];          // appended rows in front of object j; pre[m] = a
    int pad2;
};
static_assert(sizeof(PstPointsFrame) % 8 == 0, "table rows stay 8-byte aligned");

struct PstPatchRec {
    int x0, y0, w, h;                  // destination rectangle, clipped to the image
    int sx, sy, pw, ph;                // offset of its first pixel inside the patch; the patch's width and height
    long long start;                   // first byte of the patch [3][ph][pw] in the bank
};
struct PstPatchFrame {
    int m, pad;
    PstPatchRec r[PST_REC_MAX];
};

// a thread moves its PST_ITEMS rows (strided by the block, as k_augment_points_b): a source row against the frame's m records, or
// a bank row.  Reads and writes are dwords: nothing beyond 4-byte alignment is known of a frame, the bank or the output.
__device__ __forceinline__ void pst_points(const PstPointsFrame &f, const unsigned *__restrict__ bank)
{
    const int n = f.n, m = f.m, total = n + f.a;
    const unsigned *__restrict__ pts = f.pts;
    unsigned *__restrict__ out = f.out;
    const long long base = (long long)blockIdx.x * PST_TILE + threadIdx.x;
    if (base >= total) return;
    unsigned x[PST_ITEMS], y[PST_ITEMS], z[PST_ITEMS];
    bool gone[PST_ITEMS];
#pragma unroll
    for (int k = 0; k < PST_ITEMS; ++k) {
        const long long i = base + k * PST_THREADS;
        x[k] = y[k] = z[k] = 0u;
        gone[k] = false;
        if (i < n) {
            const unsigned *q = pts + 3 * (size_t)i;
            x[k] = q[0]; y[k] = q[1]; z[k] = q[2];
        } else if (i < total) {
            const int t = (int)(i - n);
            int j = 0;
            while (j + 1 < m && f.pre[j + 1] <= t) ++j;
            const unsigned *q = bank + 3 * ((size_t)f.start[j] + (size_t)(t - f.pre[j]));
            x[k] = q[0]; y[k] = q[1]; z[k] = q[2];
        }
    }
    if (base < n) {
        // a record is fetched once (wave-uniform) for the thread's rows; rows that are the bank's, or beyond the end, are skipped
        for (int j = 0; j < m; ++j) {
            const float cx = f.rec[j][0], cy = f.rec[j][1], cz = f.rec[j][2], c = f.rec[j][3], s = f.rec[j][4];
            const float hl = f.rec[j][5], hw = f.rec[j][6], hh = f.rec[j][7];
#pragma unroll
            for (int k = 0; k < PST_ITEMS; ++k) {
                const float dx = __fsub_rn(__uint_as_float(x[k]), cx), dy = __fsub_rn(__uint_as_float(y[k]), cy);
                const float lx = __fadd_rn(__fmul_rn(dx, c), __fmul_rn(dy, s));
                const float ly = __fsub_rn(__fmul_rn(dy, c), __fmul_rn(dx, s));
                const bool in = fabsf(lx) <= hl && fabsf(ly) <= hw && fabsf(__fsub_rn(__uint_as_float(z[k]), cz)) <= hh;    // NaN / inf: false
                gone[k] = gone[k] || (in && base + k * PST_THREADS < n);
            }
        }
    }
    const unsigned inf = 0x7f800000u;
#pragma unroll
    for (int k = 0; k < PST_ITEMS; ++k) {
        const long long i = base + k * PST_THREADS;
        if (i < total) {
            unsigned *o = out + 3 * (size_t)i;
            o[0] = gone[k] ? inf : x[k]; o[1] = gone[k] ? inf : y[k]; o[2] = gone[k] ? inf : z[k];
        }
    }
}

// A thread produces the 4 bytes of one ALIGNED dword of the output (the dword grid of k_augment_image_b: laid from the frame's
// first byte rounded down to 4, so nothing is assumed about the alignment of `out`, of a frame, of a plane or of a row).  Whole
// dwords go out as one store; the dwords a frame shares with its neighbours go out in byte stores of the frame's own bytes only.
// Each byte is the owning record's patch byte or the input byte: no thread reads what another writes.
__device__ __forceinline__ void pst_patches(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const PstPatchFrame &f, const uint8_t *__restrict__ bank,
                                            int H, int W)
{
    const int b = blockIdx.y;
    const int m = f.m;
    const int hw = H * W, N = 3 * hw;                              // N <= 2^30: checked on the host
    in += (size_t)b * N;
    out += (size_t)b * N;
    const int mis = (int)((uintptr_t)out & 3);
    const long long first = ((long long)blockIdx.x * PST_THREADS + threadIdx.x) * 4 - mis;     // flat index of this dword's byte 0 (-3 .. N-1)
    if (first >= N) return;
    const int kstart = first < 0 ? (int)-first : 0;
    const int i0 = (int)first + kstart;
    int c = i0 / hw;
    const int r0 = i0 - c * hw;
    int h = r0 / W;
    int w = r0 - h * W;
    // (c, h, w) of the thread's live bytes, then the owner of each: the LAST listed record whose rectangle contains it.  A record
    // is fetched once (wave-uniform) for the four bytes
    int ck[4], hk[4], wk[4], own[4];
    bool live[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        live[k] = k >= kstart && first + k < N;
        ck[k] = c; hk[k] = h; wk[k] = w; own[k] = -1;
        if (live[k] && ++w == W) {
            w = 0;
            if (++h == H) { h = 0; ++c; }
        }
    }
    for (int j = 0; j < m; ++j) {
        const int x0 = f.r[j].x0, y0 = f.r[j].y0, rw = f.r[j].w, rh = f.r[j].h;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((unsigned)(wk[k] - x0) < (unsigned)rw && (unsigned)(hk[k] - y0) < (unsigned)rh) own[k] = j;
    }
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (live[k]) {
            unsigned v;
            if (own[k] >= 0) {
                const PstPatchRec &r = f.r[own[k]];
                v = bank[(size_t)r.start + ((size_t)ck[k] * r.ph + (size_t)(hk[k] - r.y0 + r.sy)) * r.pw + (size_t)(wk[k] - r.x0 + r.sx)];
            } else {
                v = in[first + k];
            }
            word |= v << (8 * k);
        }
    }
    if (kstart == 0 && first + 3 < N) {
        *reinterpret_cast<unsigned *>(out + first) = word;          // (out - mis) is 4-byte aligned and first = 4 t - mis
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k >= kstart && first + k < N) out[first + k] = (uint8_t)(word >> (8 * k));
    }
}

// Two ways for a frame's table to reach its blocks.  Up to PST_VALUE_MAX frames (the cfg2 batch has two) the tables fit the 4 KB a
// kernel takes by value and are read straight from the kernel argument -- the index is wave-uniform, the loads are scalar loads of
// the argument segment, no scratch.  More frames (5 .. 8) read a table the host staged in device memory in front of the launch.
constexpr int PST_VALUE_MAX = 4;
struct PstPointsArg { PstPointsFrame f[PST_VALUE_MAX]; };
struct PstPatchArg { PstPatchFrame f[PST_VALUE_MAX]; };
static_assert(sizeof(PstPointsArg) + 8 <= 4096 && sizeof(PstPatchArg) + 40 <= 4096, "by-value tables fit a kernel argument");

__global__ void __launch_bounds__(PST_THREADS) k_paste_points_v(PstPointsArg a, const unsigned *__restrict__ bank) { pst_points(a.f[blockIdx.y], bank); }
__global__ void __launch_bounds__(PST_THREADS) k_paste_points_b(const PstPointsFrame *__restrict__ tab, const unsigned *__restrict__ bank)
{
    pst_points(tab[blockIdx.y], bank);
}
__global__ void __launch_bounds__(PST_THREADS) k_paste_patches_v(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, PstPatchArg a,
                                                                 const uint8_t *__restrict__ bank, int H, int W)
{
    pst_patches(in, out, a.f[blockIdx.y], bank, H, W);
}
__global__ void __launch_bounds__(PST_THREADS) k_paste_patches_b(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const PstPatchFrame *__restrict__ tab,
                                                                 const uint8_t *__restrict__ bank, int H, int W)
{
    pst_patches(in, out, tab[blockIdx.y], bank, H, W);
}

inline bool pst_apart(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a1 <= b0 || b1 <= a0 || a0 == a1 || b0 == b1; }

}  // namespace

// Points of object pasting for the B (<= 8) frames of a batch in one launch.  pts / n / m / rec / app / out / out_rows: HOST arrays
// (B device pointers, B row counts, B record counts <= 16, B x 16 x 8 records, B x 16 x (bank start, count), B device pointers, B
// output capacities in rows).  bank: device fp32 [bank_rows][3].  stage_host / stage_dev (needed for B > 4 only): stage_bytes (>= 8192)
// of pinned host memory and of device memory that stay untouched until the stream has passed this call.  An output overlaps no input and no
// other output.  Bit for bit paste.paste_points per frame; nothing is written beyond row n + a of an output.
extern "C" int dcf_paste_points_batch(const float *const *pts, const int *n, int B, const int *m, const float *rec, const int64_t *app,
                                      const float *bank, int64_t bank_rows, float *const *out, const int *out_rows, void *stage_host,
                                      void *stage_dev, size_t stage_bytes, dcf_stream_t stream)
{
    const char *who = "dcf_paste_points_batch";
    DCF_REQUIRE(pts && n && m && rec && app && out && out_rows, "%s: bad arguments", who);
    DCF_REQUIRE(B >= 1 && B <= PST_BATCH_MAX, "%s: 1..%d frames per call", who, PST_BATCH_MAX);
    DCF_REQUIRE(bank_rows >= 0 && bank_rows <= INT_MAX && (bank || bank_rows == 0), "%s: bad bank", who);
    const bool staged = B > PST_VALUE_MAX;
    DCF_REQUIRE(!staged || (stage_host && stage_dev && stage_bytes >= sizeof(PstPointsFrame) * PST_BATCH_MAX && ((uintptr_t)stage_host & 7) == 0 &&
                            ((uintptr_t)stage_dev & 7) == 0),
                "%s: more than %d frames need staging buffers of at least %zu bytes, 8-byte aligned", who, PST_VALUE_MAX, sizeof(PstPointsFrame) * PST_BATCH_MAX);
    DCF_REQUIRE(((uintptr_t)bank & 3) == 0, "%s: bank must be 4-byte aligned", who);
    PstPointsArg arg;
    PstPointsFrame *tab = staged ? (PstPointsFrame *)stage_host : arg.f;
    int64_t rows_max = 0;
    double bytes = 0.0;
    uintptr_t lo[2 * PST_BATCH_MAX], hi[2 * PST_BATCH_MAX];          // ranges: inputs, then outputs
    for (int b = 0; b < B; ++b) {
        DCF_REQUIRE(n[b] >= 0 && m[b] >= 0 && m[b] <= PST_REC_MAX, "%s: frame %d: bad point / record count", who, b);
        DCF_REQUIRE(n[b] == 0 || pts[b], "%s: frame %d: null points", who, b);
        int64_t a = 0;
        for (int j = 0; j < m[b]; ++j) {
            const int64_t s = app[(b * PST_REC_MAX + j) * 2], c = app[(b * PST_REC_MAX + j) * 2 + 1];
            DCF_REQUIRE(s >= 0 && c >= 0 && c <= bank_rows && s <= bank_rows - c, "%s: frame %d: object %d outside the bank", who, b, j);
            a += c;
        }
        const int64_t rows = (int64_t)n[b] + a;
        DCF_REQUIRE(rows <= out_rows[b] && rows <= INT_MAX / 4, "%s: frame %d: %lld rows for an output of %d", who, b, (long long)rows, out_rows[b]);
        DCF_REQUIRE(rows == 0 || out[b], "%s: frame %d: null output", who, b);
        DCF_REQUIRE(((((uintptr_t)pts[b]) | ((uintptr_t)out[b])) & 3) == 0, "%s: frame %d: pointers must be 4-byte aligned", who, b);
        lo[b] = (uintptr_t)pts[b]; hi[b] = lo[b] + 12 * (uintptr_t)n[b];
        lo[PST_BATCH_MAX + b] = (uintptr_t)out[b]; hi[PST_BATCH_MAX + b] = lo[PST_BATCH_MAX + b] + 12 * (uintptr_t)rows;
        if (rows > rows_max) rows_max = rows;
        bytes += 24.0 * (double)rows;
    }
    const uintptr_t k0 = (uintptr_t)bank, k1 = k0 + 12 * (uintptr_t)bank_rows;
    for (int b = 0; b < B; ++b) {
        const uintptr_t o0 = lo[PST_BATCH_MAX + b], o1 = hi[PST_BATCH_MAX + b];
        DCF_REQUIRE(pst_apart(o0, o1, k0, k1), "%s: output of frame %d overlaps the bank", who, b);
        for (int c = 0; c < B; ++c) {
            DCF_REQUIRE(pst_apart(o0, o1, lo[c], hi[c]), "%s: output of frame %d overlaps the input of frame %d", who, b, c);
            DCF_REQUIRE(b == c || pst_apart(o0, o1, lo[PST_BATCH_MAX + c], hi[PST_BATCH_MAX + c]), "%s: outputs of frames %d and %d overlap", who, b, c);
        }
    }
    if (rows_max == 0) return DCF_OK;
    memset(tab, 0, sizeof(PstPointsFrame) * (staged ? PST_BATCH_MAX : PST_VALUE_MAX));
    for (int b = 0; b < B; ++b) {
        PstPointsFrame &f = tab[b];
        f.pts = (const unsigned *)pts[b];
        f.out = (unsigned *)out[b];
        f.n = n[b];
        f.m = m[b];
        int a = 0;
        for (int j = 0; j < m[b]; ++j) {
            for (int k = 0; k < 8; ++k) f.rec[j][k] = rec[(b * PST_REC_MAX + j) * 8 + k];
            f.start[j] = (int)app[(b * PST_REC_MAX + j) * 2];
            f.pre[j] = a;
            a += (int)app[(b * PST_REC_MAX + j) * 2 + 1];
        }
        for (int j = m[b]; j <= PST_REC_MAX; ++j) f.pre[j] = a;
        f.a = a;
    }
    hipStream_t s = S(stream);
    const dim3 grid(cdiv(rows_max, PST_TILE), B);
    if (!staged) {
        DCF_LAUNCH_B("paste_points", bytes, s, hipLaunchKernelGGL(k_paste_points_v, grid, dim3(PST_THREADS), 0, s, arg, (const unsigned *)bank));
        return DCF_OK;
    }
    DCF_HIP(hipMemcpyAsync(stage_dev, stage_host, sizeof(PstPointsFrame) * B, hipMemcpyHostToDevice, s));
    DCF_LAUNCH_B("paste_points", bytes, s,
                 hipLaunchKernelGGL(k_paste_points_b, grid, dim3(PST_THREADS), 0, s, (const PstPointsFrame *)stage_dev, (const unsigned *)bank));
    return DCF_OK;
}

// Patches of object pasting for the B (<= 8) frames of a batch in one launch.  img / out: device uint8 [B][3][H][W], contiguous, any
// byte alignment, not overlapping; m / rec: HOST arrays (B record counts <= 16, B x 16 x 9 = {x0, y0, w, h, sx, sy, pw, ph, start});
// bank: device uint8 [bank_bytes]; the staging buffers as in dcf_paste_points_batch.  Byte for byte paste.paste_image per frame.
extern "C" int dcf_paste_patches_batch(const uint8_t *img, int B, int H, int W, const int *m, const int64_t *rec, const uint8_t *bank,
                                       int64_t bank_bytes, uint8_t *out, void *stage_host, void *stage_dev, size_t stage_bytes, dcf_stream_t stream)
{
    const char *who = "dcf_paste_patches_batch";
    DCF_REQUIRE(img && m && rec && out, "%s: bad arguments", who);
    DCF_REQUIRE(B >= 1 && B <= PST_BATCH_MAX, "%s: 1..%d frames per call", who, PST_BATCH_MAX);
    DCF_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= (int64_t)(1 << 30) / 3, "%s: H, W >= 1 and 3 H W <= 2^30 (got %d x %d)", who, H, W);
    DCF_REQUIRE(bank_bytes >= 0 && (bank || bank_bytes == 0), "%s: bad bank", who);
    const bool staged = B > PST_VALUE_MAX;
    DCF_REQUIRE(!staged || (stage_host && stage_dev && stage_bytes >= sizeof(PstPatchFrame) * PST_BATCH_MAX && ((uintptr_t)stage_host & 7) == 0 &&
                            ((uintptr_t)stage_dev & 7) == 0),
                "%s: more than %d frames need staging buffers of at least %zu bytes, 8-byte aligned", who, PST_VALUE_MAX, sizeof(PstPatchFrame) * PST_BATCH_MAX);
    const size_t frame = (size_t)3 * H * W, total = frame * B;
    const uintptr_t i0 = (uintptr_t)img, o0 = (uintptr_t)out, k0 = (uintptr_t)bank;
    DCF_REQUIRE(i0 + total <= o0 || o0 + total <= i0, "%s: out overlaps the input", who);
    DCF_REQUIRE(bank_bytes == 0 || k0 + (uintptr_t)bank_bytes <= o0 || o0 + total <= k0, "%s: out overlaps the bank", who);
    for (int b = 0; b < B; ++b) {
        DCF_REQUIRE(m[b] >= 0 && m[b] <= PST_REC_MAX, "%s: frame %d: bad record count", who, b);
        for (int j = 0; j < m[b]; ++j) {
            const int64_t *q = rec + (b * PST_REC_MAX + j) * 9;
            DCF_REQUIRE(q[2] >= 1 && q[3] >= 1 && q[0] >= 0 && q[1] >= 0 && q[0] <= W - q[2] && q[1] <= H - q[3],
                        "%s: frame %d: record %d: destination outside the image", who, b, j);
            DCF_REQUIRE(q[6] >= 1 && q[7] >= 1 && q[6] <= W && q[7] <= H && q[4] >= 0 && q[5] >= 0 && q[4] <= q[6] - q[2] && q[5] <= q[7] - q[3],
                        "%s: frame %d: record %d: source outside its patch", who, b, j);
            DCF_REQUIRE(q[8] >= 0 && 3 * q[6] * q[7] <= bank_bytes && q[8] <= bank_bytes - 3 * q[6] * q[7], "%s: frame %d: record %d: patch outside the bank", who, b, j);
        }
    }
    PstPatchArg arg;
    PstPatchFrame *tab = staged ? (PstPatchFrame *)stage_host : arg.f;
    memset(tab, 0, sizeof(PstPatchFrame) * (staged ? PST_BATCH_MAX : PST_VALUE_MAX));
    for (int b = 0; b < B; ++b) {
        tab[b].m = m[b];
        for (int j = 0; j < m[b]; ++j) {
            const int64_t *q = rec + (b * PST_REC_MAX + j) * 9;
            PstPatchRec &r = tab[b].r[j];
            r.x0 = (int)q[0]; r.y0 = (int)q[1]; r.w = (int)q[2]; r.h = (int)q[3];
            r.sx = (int)q[4]; r.sy = (int)q[5]; r.pw = (int)q[6]; r.ph = (int)q[7];
            r.start = q[8];
        }
    }
    hipStream_t s = S(stream);
    const dim3 grid(cdiv((int64_t)frame + 3, PST_THREADS * 4), B);
    if (!staged) {
        DCF_LAUNCH_B("paste_patches", 2.0 * (double)total, s, hipLaunchKernelGGL(k_paste_patches_v, grid, dim3(PST_THREADS), 0, s, img, out, arg, bank, H, W));
        return DCF_OK;
    }
    DCF_HIP(hipMemcpyAsync(stage_dev, stage_host, sizeof(PstPatchFrame) * B, hipMemcpyHostToDevice, s));
    DCF_LAUNCH_B("paste_patches", 2.0 * (double)total, s,
                 hipLaunchKernelGGL(k_paste_patches_b, grid, dim3(PST_THREADS), 0, s, img, out, (const PstPatchFrame *)stage_dev, bank, H, W));
    return DCF_OK;
}
