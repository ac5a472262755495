// camera_mask.hip -- the camera visibility mask (host statement: visibility.py).
//
// One launch over the frames of a batch (blockIdx.y = frame): a row of a frame that the camera cannot see is overwritten with
// (+inf, +inf, +inf), the convention of the point drop and of object pasting -- every range test rejects such a row, nothing is
// compacted, the point counts stay host-known.  Two rules, either or both per launch:
//   fov         the row fails the projection's own predicate (ProjPred, proj_pred.h) under the frame's matrix
//   occluders   the row projects into one of the frame's (<= 16) rectangles and lies deeper than that rectangle's depth D
// A frame's table (pointers, counts, 12 matrix floats, 16 x 5 occluder floats) is 392 bytes, eight of them fit the 4 KB a kernel
// takes by value: everything travels in the kernel argument, no staging copy at any batch size.  The frame index is wave-uniform
// and the table is read with scalar loads of the argument segment (no scratch: the compiler's resource remarks, section 23).
//
// Bit-exactness contract: u, v and a2 are ProjPred's chain (__fmul_rn / __fmaf_rn / __fdiv_rn, the file is built with
// -ffp-contract=off like the rest of the library); the compares are fp32.  Rows are moved as dwords: a NaN keeps its payload.
#include <limits.h>
#include <math.h>

#include "dcf_common.h"
#include "proj_pred.h"

namespace {

constexpr int CM_BATCH_MAX = 8;        // frames per launch (DCF_PROJ_BATCH_MAX of geometry.hip)
constexpr int CM_OCC_MAX = 16;         // occluders per frame: one per patch record of a paste plan
constexpr int CM_THREADS = 256;
constexpr int CM_ITEMS = 4;
constexpr int CM_TILE = CM_THREADS * CM_ITEMS;

struct CmFrame {
    const unsigned *pts;
    unsigned *out;
    int n, m;
    Crt12 c;
    float occ[CM_OCC_MAX][5];          // x0 y0 x1 y1 D
};
struct CmArg { CmFrame f[CM_BATCH_MAX]; };
static_assert(sizeof(CmFrame) % 8 == 0, "table rows stay 8-byte aligned");
static_assert(sizeof(CmArg) + sizeof(Lim6) + 16 <= 4096, "the tables fit a kernel argument");

// a thread loads its CM_ITEMS rows (strided by the block, as k_augment_points_b), decides, then stores them: it reads and writes
// its own rows only, so out == pts is allowed.  Dword accesses: nothing beyond 4-byte alignment is known of a frame.
__global__ void __launch_bounds__(CM_THREADS) k_camera_mask_b(CmArg a, Lim6 lim, float ulim, float vlim, int mode, int fov)
{
    const CmFrame &f = a.f[blockIdx.y];
    const int n = f.n, m = f.m;
    const long long base = (long long)blockIdx.x * CM_TILE + threadIdx.x;
    if (base >= n) return;
    const unsigned *__restrict__ pts = f.pts;
    unsigned *__restrict__ out = f.out;
    unsigned x[CM_ITEMS], y[CM_ITEMS], z[CM_ITEMS];
#pragma unroll
    for (int k = 0; k < CM_ITEMS; ++k) {
        const long long i = base + k * CM_THREADS;
        x[k] = y[k] = z[k] = 0u;
        if (i < n) {
            const unsigned *q = pts + 3 * (size_t)i;
            x[k] = q[0]; y[k] = q[1]; z[k] = q[2];
        }
    }
    ProjPred pred;
    pred.lim = lim; pred.c = f.c; pred.ulim = ulim; pred.vlim = vlim; pred.mode = mode;
    float u[CM_ITEMS], v[CM_ITEMS], a2[CM_ITEMS];
    bool gone[CM_ITEMS];
#pragma unroll
    for (int k = 0; k < CM_ITEMS; ++k) {
        const float row[3] = {__uint_as_float(x[k]), __uint_as_float(y[k]), __uint_as_float(z[k])};
        proj_chain(row[0], row[1], row[2], pred.c, u[k], v[k], a2[k]);
        float pu, pv;
        gone[k] = fov != 0 && !pred(row, 0, &pu, &pv);
    }
    // an occluder is fetched once (wave-uniform) for the thread's rows; a NaN compares false
    for (int j = 0; j < m; ++j) {
        const float x0 = f.occ[j][0], y0 = f.occ[j][1], x1 = f.occ[j][2], y1 = f.occ[j][3], D = f.occ[j][4];
#pragma unroll
        for (int k = 0; k < CM_ITEMS; ++k)
            gone[k] = gone[k] || (u[k] >= x0 && u[k] < x1 && v[k] >= y0 && v[k] < y1 && a2[k] > D);
    }
    const unsigned inf = 0x7f800000u;
#pragma unroll
    for (int k = 0; k < CM_ITEMS; ++k) {
        const long long i = base + k * CM_THREADS;
        if (i < n) {
            unsigned *o = out + 3 * (size_t)i;
            o[0] = gone[k] ? inf : x[k]; o[1] = gone[k] ? inf : y[k]; o[2] = gone[k] ? inf : z[k];
        }
    }
}

}  // namespace

// The camera visibility mask for the B (<= 8) frames of a batch in one launch.  pts / n / crt / m / occ / out: HOST arrays (B device
// pointers, B row counts, B x 12 matrix floats, B occluder counts <= 16, B x 16 x {x0, y0, x1, y1, D}, B device pointers).  out[b] ==
// pts[b] is allowed, every other overlap of an output with an input or another output is refused, as is an occluder with a
// non-finite number or an empty-side rectangle turned inside out (x1 < x0, y1 < y0).  Bit for bit visibility.mask_points per
// frame; nothing is written beyond row n[b].
extern "C" int dcf_camera_mask_points_batch(const float *const *pts, const int *n, int B, const float *lim, const float *crt, float ulim, float vlim,
                                            int mode, int fov, const int *m, const float *occ, float *const *out, dcf_stream_t stream)
{
    const char *who = "dcf_camera_mask_points_batch";
    DCF_REQUIRE(pts && n && lim && crt && m && out, "%s: bad arguments", who);
    DCF_REQUIRE(B >= 1 && B <= CM_BATCH_MAX, "%s: 1..%d frames per call", who, CM_BATCH_MAX);
    DCF_REQUIRE(mode == DCF_PROJ_COMPAT || mode == DCF_PROJ_CORRECT, "%s: bad projection mode %d", who, mode);
    CmArg arg;
    memset(&arg, 0, sizeof(arg));
    int nmax = 0;
    double total = 0.0;
    for (int b = 0; b < B; ++b) {
        DCF_REQUIRE(n[b] >= 0 && (n[b] == 0 || (pts[b] && out[b])), "%s: frame %d: bad point count / null points", who, b);
        DCF_REQUIRE(((((uintptr_t)pts[b]) | ((uintptr_t)out[b])) & 3) == 0, "%s: frame %d: pointers must be 4-byte aligned", who, b);
        DCF_REQUIRE(m[b] >= 0 && m[b] <= CM_OCC_MAX && (m[b] == 0 || occ), "%s: frame %d: 0..%d occluders", who, b, CM_OCC_MAX);
        CmFrame &f = arg.f[b];
        f.pts = (const unsigned *)pts[b];
        f.out = (unsigned *)out[b];
        f.n = n[b];
        f.m = m[b];
        memcpy(f.c.v, crt + 12 * b, sizeof(f.c.v));
        for (int j = 0; j < m[b]; ++j) {
            const float *q = occ + ((size_t)b * CM_OCC_MAX + j) * 5;
            for (int k = 0; k < 5; ++k) {
                DCF_REQUIRE(isfinite(q[k]), "%s: frame %d: occluder %d: non-finite number", who, b, j);
                f.occ[j][k] = q[k];
            }
            DCF_REQUIRE(q[2] >= q[0] && q[3] >= q[1], "%s: frame %d: occluder %d: rectangle inside out", who, b, j);
        }
        if (n[b] > nmax) nmax = n[b];
        total += n[b];
    }
    // an output may alias its own frame's input exactly; every other overlap of an output with an input or another output is a race
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < B; ++c) {
            if (!n[b] || !n[c]) continue;
            const uintptr_t o0 = (uintptr_t)out[b], o1 = o0 + 12 * (uintptr_t)n[b];
            const uintptr_t p0 = (uintptr_t)pts[c], p1 = p0 + 12 * (uintptr_t)n[c];
            const uintptr_t q0 = (uintptr_t)out[c], q1 = q0 + 12 * (uintptr_t)n[c];
            DCF_REQUIRE((b == c && o0 == p0) || o1 <= p0 || p1 <= o0, "%s: output of frame %d overlaps the input of frame %d", who, b, c);
            DCF_REQUIRE(b == c || o1 <= q0 || q1 <= o0, "%s: outputs of frames %d and %d overlap", who, b, c);
        }
    if (nmax == 0) return DCF_OK;
    Lim6 l;
    memcpy(l.v, lim, sizeof(l.v));
    hipStream_t s = S(stream);
    DCF_LAUNCH_B("camera_mask", total * 24.0, s,
                 hipLaunchKernelGGL(k_camera_mask_b, dim3(cdiv(nmax, CM_TILE), B), dim3(CM_THREADS), 0, s, arg, l, ulim, vlim, mode, fov));
    return DCF_OK;
}
