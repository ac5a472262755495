// amp.hip -- the guarded optimiser step: loss scaling (static, or torch.amp.GradScaler's dynamic schedule), exact skip of a
// step whose gradient holds a NaN / inf, and global-norm gradient clipping, all decided on the device (train.py:28,36 of the
// reference: its Adam step, with the guards fp16 training relies on).  Three dependent launches on one stream:
//   k_grad_stats    one read of the fp32 gradient arena: per-workgroup non-finite flag and fp32 partial sum of g^2
//   k_amp_update    one workgroup: fixed-order reduction, found_inf, norm / clip coefficient, GradScaler's scale rule,
//                   step counters, the step's Adam scalars
//   k_adam_guarded  k_adam's arithmetic with the scalars read from the state; nothing is stored when found_inf is set
// The grid of k_grad_stats is fixed (DCF_AMP_PARTS workgroups, grid-stride), so the norm is the same bits on every device.
// State is written by one lane with plain stores; no atomics (the launches are ordered on the stream).
#include "dcf_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;

// exponent field all ones <=> inf or NaN; an integer test, which no floating-point relaxation can fold away
__device__ __forceinline__ unsigned expo(float x) { return __float_as_uint(x) & 0x7f800000u; }
constexpr unsigned kExpAllOnes = 0x7f800000u;

__device__ __forceinline__ bool finite_bits(float x) { return expo(x) != kExpAllOnes; }

// fixed-shape reductions over a 256-thread workgroup (4 waves of 64): shuffle tree inside a wave, then the 4 wave results in
// wave order -- the same order on every launch
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ unsigned wave_max(unsigned v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ void acc4(float4 x, float &s, unsigned &e)
{
    s = s + x.x * x.x;
    s = s + x.y * x.y;
    s = s + x.z * x.z;
    s = s + x.w * x.w;
    unsigned a = expo(x.x), b = expo(x.y), c = expo(x.z), d = expo(x.w);
    a = a > b ? a : b;
    c = c > d ? c : d;
    a = a > c ? a : c;
    e = e > a ? e : a;
}

}  // namespace

__global__ void __launch_bounds__(kThreads) k_grad_stats(const float *__restrict__ g, int64_t n, dcf_amp_state *st)
{
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)DCF_AMP_PARTS * kThreads;
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    float s = 0.f;
    unsigned e = 0u;            // largest exponent field seen
    int64_t i = t;
    for (; i + 3 * stride < n4; i += 4 * stride) {      // four independent 16-byte loads in flight per lane
        const float4 a = g4[i], b = g4[i + stride], c = g4[i + 2 * stride], d = g4[i + 3 * stride];
        acc4(a, s, e);
        acc4(b, s, e);
        acc4(c, s, e);
        acc4(d, s, e);
    }
    for (; i < n4; i += stride) acc4(g4[i], s, e);
    if (t < (n & 3)) {                                   // ragged tail: at most 3 elements, one per lane of workgroup 0
        const float x = g[n4 * 4 + t];
        s = s + x * x;
        const unsigned a = expo(x);
        e = e > a ? e : a;
    }
    __shared__ float red_s[kThreads / 64];
    __shared__ unsigned red_e[kThreads / 64];
    s = wave_sum(s);
    e = wave_max(e);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_s[w] = s;
        red_e[w] = e;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float tot = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
        unsigned em = red_e[0];
        for (int k = 1; k < kThreads / 64; ++k) em = red_e[k] > em ? red_e[k] : em;
        st->part_sum[blockIdx.x] = tot;
        st->part_flag[blockIdx.x] = em == kExpAllOnes ? 1 : 0;
        // the scale this step's backward was seeded with (the seed reads scale_next): latched here, before dcf_amp_update
        // writes the next one, so that the update never reads a field it writes
        if (blockIdx.x == 0) st->scale_in = st->scale_next;
    }
}

__global__ void __launch_bounds__(kThreads) k_amp_update(dcf_amp_state *st, float gscale_host, int dynamic, double growth_factor,
                                                         double backoff_factor, int growth_interval, float max_norm, float lr,
                                                         float beta1, float beta2)
{
    double s = 0.0;
    int f = 0;
#pragma unroll
    for (int k = 0; k < DCF_AMP_PARTS / kThreads; ++k) {
        s += (double)st->part_sum[threadIdx.x + k * kThreads];
        f |= st->part_flag[threadIdx.x + k * kThreads];
    }
    __shared__ double red_s[kThreads / 64];
    __shared__ int red_f[kThreads / 64];
    s = wave_sum(s);
    f = (int)wave_max((unsigned)f);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_s[w] = s;
        red_f[w] = f;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double sum = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    const int flag = red_f[0] | red_f[1] | red_f[2] | red_f[3];
    const float S = st->scale_in;
    const bool clip = max_norm > 0.f;
    // norm of the gradient Adam would see: the arena holds S * (sum over ranks) of the gradient, Adam multiplies by gscale_host / S
    const float norm = (float)(sqrt(sum) * fabs((double)gscale_host) / (double)S);
    const int found = flag || (clip && !finite_bits(norm));
    float coef = 1.f;
    if (clip && !found) {
        const float c = max_norm / (norm + 1e-6f);
        coef = c < 1.f ? c : 1.f;
    }
    // torch._amp_update_scale_ (aten/src/ATen/native/cuda/AmpKernels.cu): the static scale never moves
    float next = S;
    int tracker = st->growth_tracker;
    if (found) {
        if (dynamic) {
            next = (float)((double)S * backoff_factor);
            tracker = 0;
        }
        st->skipped_steps = st->skipped_steps + 1;
    } else {
        if (dynamic) {
            const int ok = tracker + 1;
            if (ok == growth_interval) {
                const float grown = (float)((double)S * growth_factor);
                if (finite_bits(grown)) next = grown;
                tracker = 0;
            } else {
                tracker = ok;
            }
        }
        const int64_t t = st->applied_steps + 1;
        st->applied_steps = t;
        // dcf_adam_step's host expressions, with the APPLIED step count: the same double arithmetic, rounded to float once
        const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
        st->lr_over_bc1 = (float)(lr / bc1);
        st->inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
        st->gscale = gscale_host / S * coef;
    }
    st->found_inf = found;
    st->grad_norm = norm;
    st->clip_coef = coef;
    st->growth_tracker = tracker;
    st->scale_next = next;
}

// k_adam (elementwise.hip) with lr / bc1, 1 / sqrt(bc2) and the gradient scale read from the state: the same expressions in the
// same order (-ffp-contract=off), so a guarded step with the same scalars stores the same bits
__global__ void __launch_bounds__(256) k_adam_guarded(float *p, const float *g, float *m, float *v, int64_t n, float b1, float b2,
                                                      float eps, const dcf_amp_state *st)
{
    if (st->found_inf) return;
    const float lr_over_bc1 = st->lr_over_bc1, inv_sqrt_bc2 = st->inv_sqrt_bc2, gscale = st->gscale;
    const int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= n) return;
    if (i4 + 4 <= n) {
        float4 pp = ld4(p + i4), gg = ld4(g + i4), mm = ld4(m + i4), vv = ld4(v + i4);
        float *P = &pp.x, *G = &gg.x, *M = &mm.x, *V = &vv.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gk = G[k] * gscale;
            M[k] = b1 * M[k] + (1.f - b1) * gk;
            V[k] = b2 * V[k] + (1.f - b2) * gk * gk;
            P[k] -= lr_over_bc1 * M[k] / (sqrtf(V[k]) * inv_sqrt_bc2 + eps);
        }
        st4(p + i4, pp); st4(m + i4, mm); st4(v + i4, vv);
    } else {
        for (int64_t i = i4; i < n; ++i) {
            const float gk = g[i] * gscale;
            m[i] = b1 * m[i] + (1.f - b1) * gk;
            v[i] = b2 * v[i] + (1.f - b2) * gk * gk;
            p[i] -= lr_over_bc1 * m[i] / (sqrtf(v[i]) * inv_sqrt_bc2 + eps);
        }
    }
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int dcf_grad_stats(const float *grads, int64_t n, dcf_amp_state *state, dcf_stream_t stream)
{
    DCF_REQUIRE(state && n >= 0 && (grads || n == 0) && aligned16(grads), "dcf_grad_stats: bad arguments (grads %p, n %lld, state %p)",
                (const void *)grads, (long long)n, (void *)state);
    hipStream_t s = S(stream);
    DCF_LAUNCH_B("grad_stats", (double)n * 4.0, s, hipLaunchKernelGGL(k_grad_stats, dim3(DCF_AMP_PARTS), dim3(kThreads), 0, s, grads, n, state));
    return DCF_OK;
}

extern "C" int dcf_amp_update(dcf_amp_state *state, float gscale_host, int dynamic, double growth_factor, double backoff_factor,
                              int growth_interval, float max_norm, float lr, float beta1, float beta2, dcf_stream_t stream)
{
    DCF_REQUIRE(state && gscale_host > 0.f && isfinite(gscale_host) && growth_factor > 0.0 && isfinite(growth_factor) &&
                backoff_factor > 0.0 && isfinite(backoff_factor) && growth_interval >= 1 && !(max_norm != max_norm) && isfinite(lr) &&
                beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f,
                "dcf_amp_update: bad arguments (state %p, gscale %g, growth %g, backoff %g, interval %d, max_norm %g)", (void *)state,
                (double)gscale_host, growth_factor, backoff_factor, growth_interval, (double)max_norm);
    hipStream_t s = S(stream);
    DCF_LAUNCH("amp_update", s, hipLaunchKernelGGL(k_amp_update, dim3(1), dim3(kThreads), 0, s, state, gscale_host, dynamic ? 1 : 0,
                                                   growth_factor, backoff_factor, growth_interval, max_norm, lr, beta1, beta2));
    return DCF_OK;
}

extern "C" int dcf_adam_step_guarded(float *params, const float *grads, float *m, float *v, int64_t n, float beta1, float beta2,
                                     float eps, const dcf_amp_state *state, dcf_stream_t stream)
{
    DCF_REQUIRE(params && grads && m && v && state && n >= 0, "dcf_adam_step_guarded: bad arguments (n %lld, state %p)", (long long)n,
                (const void *)state);
    if (n == 0) return DCF_OK;
    hipStream_t s = S(stream);
    DCF_LAUNCH_B("adam_guarded", (double)n * 28.0, s, hipLaunchKernelGGL(k_adam_guarded, dim3(cdiv(cdiv(n, 4), 256)), dim3(256), 0, s,
                                                                           params, grads, m, v, n, beta1, beta2, eps, state));
    return DCF_OK;
}
