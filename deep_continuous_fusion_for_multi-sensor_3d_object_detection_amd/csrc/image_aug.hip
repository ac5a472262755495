// image_aug.hip -- train-time camera image augmentation (host statement: augment_image.py).
//
// One gather kernel for the frames of a batch: zoom / shift / horizontal flip as an inverse axis-aligned affine with a two-tap
// bilinear per axis (taps outside the image contribute 0: grid_sample's padding_mode="zeros", align_corners=False), then the
// photometric line t = g_c val + bias and the uint8 quantiser.  A byte gather from a source that sits in L2 and a streaming
// store; latency / launch bound at the sizes of this detector (1.4 MB per cfg2 frame).
//
// Bit-exactness contract: every product, sum and difference is spelled __fmul_rn / __fadd_rn / __fsub_rn (and the file is built
// with -ffp-contract=off like the rest of the library), so each rounds exactly where augment_image.transform_image's np.float32
// arithmetic rounds; the quantiser is v_rndne (round half to even) and a clamp.
#include "dcf_common.h"

namespace {

constexpr int IMG_BATCH_MAX = 8;       // frames per launch (DCF_PROJ_BATCH_MAX of geometry.hip: the batch kernels share the limit)
constexpr int IMG_NQ = 8;              // ku cu kv cv g0 g1 g2 bias
constexpr int IMG_THREADS = 256;
constexpr int IMG_TILE = IMG_THREADS * 4;

struct ImgAugBatch { float q[IMG_BATCH_MAX][IMG_NQ]; };

// source coordinate of output position i of one axis: fl(fl(fl(k (i + .5)) + c) - .5), split into floor and fraction
__device__ __forceinline__ void img_tap(float k, float c, int i, int &i0, float &fr)
{
    const float f = __fsub_rn(__fadd_rn(__fmul_rn(k, __fadd_rn((float)i, 0.5f)), c), 0.5f);
    const float fl = floorf(f);
    i0 = (int)fl;                      // |f| < 2^30: checked on the host
    fr = __fsub_rn(f, fl);
}

// blockIdx.y = frame, per-frame values by value (static selection as in k_augment_points_b: a run-time index into the by-value
// argument would go through scratch).  A thread produces the 4 bytes of one ALIGNED dword of the output: the dword grid is laid
// from the frame's first byte rounded down to 4, so nothing is assumed about the alignment of `out`, of a frame (3 H W bytes),
// of a plane or of a row -- (c, h, w) is kept per byte.  Whole dwords go out as one store; the dwords a frame shares with its
// neighbours (or with the bytes around the tensor) go out in byte stores of the frame's own bytes only.
__global__ void __launch_bounds__(IMG_THREADS) k_augment_image_b(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, ImgAugBatch ab, int H, int W)
{
    const int b = blockIdx.y;
    float ku = 0.f, cu = 0.f, kv = 0.f, cv = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f, bias = 0.f;
#pragma unroll
    for (int f = 0; f < IMG_BATCH_MAX; ++f)
        if (f == b) {
            ku = ab.q[f][0]; cu = ab.q[f][1]; kv = ab.q[f][2]; cv = ab.q[f][3];
            g0 = ab.q[f][4]; g1 = ab.q[f][5]; g2 = ab.q[f][6]; bias = ab.q[f][7];
        }
    const int hw = H * W, N = 3 * hw;                              // N <= 2^30: checked on the host
    in += (size_t)b * N;
    out += (size_t)b * N;
    const int mis = (int)((uintptr_t)out & 3);
    const long long first = ((long long)blockIdx.x * IMG_THREADS + threadIdx.x) * 4 - mis;     // flat index of this dword's byte 0 (-3 .. N-1)
    if (first >= N) return;
    const int kstart = first < 0 ? (int)-first : 0;
    const int i0 = (int)first + kstart;
    int c = i0 / hw;
    const int r = i0 - c * hw;
    int h = r / W;
    int w = r - h * W;
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= kstart && first + k < N) {
            int x0, y0;
            float wx, wy;
            img_tap(ku, cu, w, x0, wx);
            img_tap(kv, cv, h, y0, wy);
            const bool xa = (unsigned)x0 < (unsigned)W, xb = (unsigned)(x0 + 1) < (unsigned)W;
            const bool ya = (unsigned)y0 < (unsigned)H, yb = (unsigned)(y0 + 1) < (unsigned)H;
            const uint8_t *pl = in + (size_t)c * hw;
            const float p00 = (ya && xa) ? (float)pl[y0 * W + x0] : 0.f;
            const float p01 = (ya && xb) ? (float)pl[y0 * W + x0 + 1] : 0.f;
            const float p10 = (yb && xa) ? (float)pl[(y0 + 1) * W + x0] : 0.f;
            const float p11 = (yb && xb) ? (float)pl[(y0 + 1) * W + x0 + 1] : 0.f;
            const float ax = __fsub_rn(1.0f, wx), ay = __fsub_rn(1.0f, wy);
            const float top = __fadd_rn(__fmul_rn(p00, ax), __fmul_rn(p01, wx));
            const float bot = __fadd_rn(__fmul_rn(p10, ax), __fmul_rn(p11, wx));
            const float val = __fadd_rn(__fmul_rn(top, ay), __fmul_rn(bot, wy));
            const float g = c == 0 ? g0 : (c == 1 ? g1 : g2);
            const float t = __fadd_rn(__fmul_rn(g, val), bias);
            const unsigned v = (unsigned)fminf(fmaxf(rintf(t), 0.f), 255.f);
            word |= v << (8 * k);
            if (++w == W) {
                w = 0;
                if (++h == H) { h = 0; ++c; }
            }
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

}  // namespace

// Train-time image augmentation of the B frames of a batch in one launch.  img / out: device uint8 [B][3][H][W], contiguous, any
// byte alignment, not overlapping (the kernel gathers neighbours); q: HOST float[B][8] = {ku, cu, kv, cv, g0, g1, g2, bias} per
// frame.  Bit for bit augment_image.transform_image per frame.
extern "C" int dcf_augment_image_batch(const uint8_t *img, int B, int H, int W, const float *q, uint8_t *out, dcf_stream_t stream)
{
    const char *who = "dcf_augment_image_batch";
    DCF_REQUIRE(img && q && out, "%s: bad arguments", who);
    DCF_REQUIRE(B >= 1 && B <= IMG_BATCH_MAX, "%s: 1..%d frames per call", who, IMG_BATCH_MAX);
    DCF_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= (int64_t)(1 << 30) / 3, "%s: H, W >= 1 and 3 H W <= 2^30 (got %d x %d)", who, H, W);
    ImgAugBatch ab;
    for (int b = 0; b < IMG_BATCH_MAX; ++b)
        for (int k = 0; k < IMG_NQ; ++k) {
            const float v = b < B ? q[IMG_NQ * b + k] : 0.f;
            DCF_REQUIRE(v == v && v - v == 0.f, "%s: frame %d: parameter %d is not finite", who, b, k);
            ab.q[b][k] = v;
        }
    for (int b = 0; b < B; ++b) {
        // the source coordinate goes to an int: keep it far inside its range
        const double mu = fabs((double)ab.q[b][0]) * (W + 1.0) + fabs((double)ab.q[b][1]);
        const double mv = fabs((double)ab.q[b][2]) * (H + 1.0) + fabs((double)ab.q[b][3]);
        DCF_REQUIRE(mu < 1073741824.0 && mv < 1073741824.0, "%s: frame %d: source coordinates beyond 2^30", who, b);
    }
    const size_t frame = (size_t)3 * H * W, total = frame * B;
    const uintptr_t i0 = (uintptr_t)img, o0 = (uintptr_t)out;
    DCF_REQUIRE(i0 + total <= o0 || o0 + total <= i0, "%s: out overlaps the input", who);
    hipStream_t s = S(stream);
    DCF_LAUNCH_B("augment_image", 2.0 * (double)total, s,
                 hipLaunchKernelGGL(k_augment_image_b, dim3(cdiv((int64_t)frame + 3, IMG_TILE), B), dim3(IMG_THREADS), 0, s, img, out, ab, H, W));
    return DCF_OK;
}
