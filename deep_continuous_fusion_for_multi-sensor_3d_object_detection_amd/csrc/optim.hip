// optim.hip -- the training recipe's optimiser step: Adam with decoupled weight decay (torch.optim.AdamW's
// p *= 1 - lr * wd in front of the update, on the tensors a one-bit-per-float4 mask names) and an exponential moving average of
// the weights, in the ONE pass that streams p, g, m, v -- plain (scalars from the host) or guarded (scalars and the skip decision
// from the dcf_amp_state of csrc/amp.hip).  Per element, fp32, nothing contracted (-ffp-contract=off), in this order:
//     gk = g * gscale
//     m' = b1*m + (1-b1)*gk            v' = b2*v + (1-b2)*gk*gk          (k_adam's expressions, elementwise.hip)
//     q  = decays(i) ? p * decay_mul : p
//     p' = q - lr_over_bc1 * m' / (sqrtf(v') * inv_sqrt_bc2 + eps)
//     e' = e + ema_omd * (p' - e)                                         (only with ema)
// With decay_mul == 1 and no ema the stores are k_adam's / k_adam_guarded's bits.  The learning-rate schedule needs nothing here:
// the host passes the step's rate by value.
// Decay mask: bit (j % 64) of word (j / 64) belongs to float4 group j = elements 4j .. 4j+3 (a tail group of fewer than four
// elements uses its bit like any other); NULL = every element decays.
// Two launch shapes, same results (option ADAMW_SHAPE, DESIGN.md section 15 has both timings):
//     flat    one group per lane, grid = groups / 256 (k_adam's shape): a wave reads exactly one mask word.  The default: at the
//             cfg2 arena size, decay + average measured 162.0 / 149.2 us (two runs) against 170.8 / 152.9 us for stride
//     stride  grid capped at 2048 workgroups, grid-stride over chunks of 512 groups, the lane's two groups (256 apart) loaded
//             before either is computed: a wave reads two mask words per chunk
// Plain C++: no inline assembly, no atomics.
#include "dcf_common.h"

#include <math.h>

struct AdamwScalars {
    float lr_over_bc1, inv_sqrt_bc2, gscale, b1, b2, eps, decay_mul, ema_omd;
};

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;          // stride shape: 256 CUs x 8 workgroups

__device__ __forceinline__ bool decays(const uint64_t *bits, int64_t group)
{
    return bits == nullptr || ((bits[group >> 6] >> (group & 63)) & 1ull) != 0;
}

__device__ __forceinline__ void update1(float &p, float g, float &m, float &v, bool dec, const AdamwScalars &c)
{
    const float gk = g * c.gscale;
    m = c.b1 * m + (1.f - c.b1) * gk;
    v = c.b2 * v + (1.f - c.b2) * gk * gk;
    const float q = dec ? p * c.decay_mul : p;
    p = q - c.lr_over_bc1 * m / (sqrtf(v) * c.inv_sqrt_bc2 + c.eps);
}

__device__ __forceinline__ float average1(float e, float p, const AdamwScalars &c) { return e + c.ema_omd * (p - e); }

__device__ __forceinline__ void update4(float4 &pp, const float4 &gg, float4 &mm, float4 &vv, bool dec, const AdamwScalars &c)
{
    update1(pp.x, gg.x, mm.x, vv.x, dec, c);
    update1(pp.y, gg.y, mm.y, vv.y, dec, c);
    update1(pp.z, gg.z, mm.z, vv.z, dec, c);
    update1(pp.w, gg.w, mm.w, vv.w, dec, c);
}

__device__ __forceinline__ float4 average4(const float4 &ee, const float4 &pp, const AdamwScalars &c)
{
    return make_float4(average1(ee.x, pp.x, c), average1(ee.y, pp.y, c), average1(ee.z, pp.z, c), average1(ee.w, pp.w, c));
}

// one group: whole (a float4 per array) or the ragged tail (element by element); group * 4 < n
template <bool EMA>
__device__ __forceinline__ void group1(float *p, const float *g, float *m, float *v, float *e, const uint64_t *bits, int64_t n,
                                       int64_t group, const AdamwScalars &c)
{
    const int64_t i4 = group * 4;
    const bool dec = decays(bits, group);
    if (i4 + 4 <= n) {
        float4 pp = ld4(p + i4), gg = ld4(g + i4), mm = ld4(m + i4), vv = ld4(v + i4), ee;
        if (EMA) ee = ld4(e + i4);
        update4(pp, gg, mm, vv, dec, c);
        st4(p + i4, pp); st4(m + i4, mm); st4(v + i4, vv);
        if (EMA) st4(e + i4, average4(ee, pp, c));
    } else {
        for (int64_t i = i4; i < n; ++i) {
            float pi = p[i], mi = m[i], vi = v[i];
            update1(pi, g[i], mi, vi, dec, c);
            p[i] = pi; m[i] = mi; v[i] = vi;
            if (EMA) e[i] = average1(e[i], pi, c);
        }
    }
}

template <bool GUARD>
__device__ __forceinline__ bool scalars(AdamwScalars &c, const dcf_amp_state *st)
{
    if (GUARD) {
        if (st->found_inf) return false;
        c.lr_over_bc1 = st->lr_over_bc1;
        c.inv_sqrt_bc2 = st->inv_sqrt_bc2;
        c.gscale = st->gscale;
    }
    return true;
}

}  // namespace

template <bool GUARD, bool EMA>
__global__ void __launch_bounds__(kThreads) k_adamw_ema_flat(float *p, const float *g, float *m, float *v, float *e, const uint64_t *bits,
                                                              int64_t n, AdamwScalars c, const dcf_amp_state *st)
{
    if (!scalars<GUARD>(c, st)) return;
    const int64_t group = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (group * 4 >= n) return;
    group1<EMA>(p, g, m, v, e, bits, n, group, c);
}

template <bool GUARD, bool EMA>
__global__ void __launch_bounds__(kThreads) k_adamw_ema_stride(float *p, const float *g, float *m, float *v, float *e, const uint64_t *bits,
                                                                int64_t n, AdamwScalars c, const dcf_amp_state *st)
{
    if (!scalars<GUARD>(c, st)) return;
    const int64_t whole = n >> 2;                       // groups of four whole elements
    const int64_t groups = (n + 3) >> 2;
    const int64_t step = (int64_t)gridDim.x * (2 * kThreads);
    int64_t base = (int64_t)blockIdx.x * (2 * kThreads);
    for (; base + 2 * kThreads <= whole; base += step) {      // both of the lane's groups whole: ten 16-byte loads in flight
        const int64_t ga = base + threadIdx.x, gb = ga + kThreads;
        const int64_t ia = ga * 4, ib = gb * 4;
        float4 pa = ld4(p + ia), ga4 = ld4(g + ia), ma = ld4(m + ia), va = ld4(v + ia), ea;
        float4 pb = ld4(p + ib), gb4 = ld4(g + ib), mb = ld4(m + ib), vb = ld4(v + ib), eb;
        if (EMA) {
            ea = ld4(e + ia);
            eb = ld4(e + ib);
        }
        const bool da = decays(bits, ga), db = decays(bits, gb);
        update4(pa, ga4, ma, va, da, c);
        st4(p + ia, pa); st4(m + ia, ma); st4(v + ia, va);
        if (EMA) st4(e + ia, average4(ea, pa, c));
        update4(pb, gb4, mb, vb, db, c);
        st4(p + ib, pb); st4(m + ib, mb); st4(v + ib, vb);
        if (EMA) st4(e + ib, average4(eb, pb, c));
    }
    if (base < groups) {                                  // the one chunk that is not whole (one workgroup gets here)
        const int64_t ga = base + threadIdx.x, gb = ga + kThreads;
        if (ga < groups) group1<EMA>(p, g, m, v, e, bits, n, ga, c);
        if (gb < groups) group1<EMA>(p, g, m, v, e, bits, n, gb, c);
    }
}

static bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static bool overlaps(const float *a, const float *b, int64_t n)
{
    return (uintptr_t)a < (uintptr_t)(b + n) && (uintptr_t)b < (uintptr_t)(a + n);
}

extern "C" int dcf_adamw_ema_step(float *params, const float *grads, float *m, float *v, float *ema, const uint64_t *decay_bits, int64_t n,
                                  float lr, float beta1, float beta2, float eps, int step, float gscale, float decay_mul, float ema_omd,
                                  const dcf_amp_state *state, dcf_stream_t stream)
{
    DCF_REQUIRE(params && grads && m && v && n >= 0 && (state || step >= 1),
                "dcf_adamw_ema_step: bad arguments (params %p, grads %p, m %p, v %p, n %lld, step %d, state %p)", (void *)params,
                (const void *)grads, (void *)m, (void *)v, (long long)n, step, (const void *)state);
    DCF_REQUIRE(aligned(params, 16) && aligned(grads, 16) && aligned(m, 16) && aligned(v, 16) && aligned(ema, 16) && aligned(decay_bits, 8),
                "dcf_adamw_ema_step: params, grads, m, v, ema must be 16-byte aligned and decay_bits 8-byte aligned");
    DCF_REQUIRE(isfinite(decay_mul) && isfinite(ema_omd) && ema_omd >= 0.f && ema_omd <= 1.f,
                "dcf_adamw_ema_step: decay_mul must be finite and ema_omd in [0, 1] (got %g, %g)", (double)decay_mul, (double)ema_omd);
    DCF_REQUIRE(!ema || !(overlaps(ema, params, n) || overlaps(ema, grads, n) || overlaps(ema, m, n) || overlaps(ema, v, n)),
                "dcf_adamw_ema_step: ema must not alias params, grads, m or v");
    if (n == 0) return DCF_OK;
    AdamwScalars c;
    c.b1 = beta1; c.b2 = beta2; c.eps = eps; c.decay_mul = decay_mul; c.ema_omd = ema_omd;
    c.lr_over_bc1 = c.inv_sqrt_bc2 = c.gscale = 0.f;
    if (!state) {                                         // dcf_adam_step's host expressions
        const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
        c.lr_over_bc1 = (float)(lr / bc1);
        c.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
        c.gscale = gscale;
    }
    static DcfOpt shape_o("ADAMW_SHAPE");
    const char *shape = shape_o.str();
    const bool stride = shape ? strcmp(shape, "stride") == 0 : false;
    const int64_t groups = (n + 3) / 4;
    const int blocks = stride ? (int)(cdiv(groups, 2 * kThreads) < kMaxBlocks ? cdiv(groups, 2 * kThreads) : kMaxBlocks) : cdiv(groups, kThreads);
    const double bytes = (double)n * (ema ? 36.0 : 28.0) + (decay_bits ? (double)n / 32.0 : 0.0);
    hipStream_t s = S(stream);
#define DCF_ADAMW(GUARD_, EMA_)                                                                                                          \
    do {                                                                                                                                  \
        if (stride)                                                                                                                       \
            DCF_LAUNCH_B("adamw_ema", bytes, s, hipLaunchKernelGGL((k_adamw_ema_stride<GUARD_, EMA_>), dim3(blocks), dim3(kThreads), 0, s, \
                                                                   params, grads, m, v, ema, decay_bits, n, c, state));                  \
        else                                                                                                                              \
            DCF_LAUNCH_B("adamw_ema", bytes, s, hipLaunchKernelGGL((k_adamw_ema_flat<GUARD_, EMA_>), dim3(blocks), dim3(kThreads), 0, s,   \
                                                                   params, grads, m, v, ema, decay_bits, n, c, state));                  \
    } while (0)
    if (state && ema) DCF_ADAMW(true, true);
    else if (state) DCF_ADAMW(true, false);
    else if (ema) DCF_ADAMW(false, true);
    else DCF_ADAMW(false, false);
#undef DCF_ADAMW
    return DCF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Parameter groups (`param_groups`): the pass above with a second side table, one BYTE per float4 group naming
// the group's id g (0 .. ngroups-1), and per id {mu, decay_mul, frozen} by value in the kernel argument:
//     frozen_g :  the float4 group is skipped -- g is not read, p, m, v, e are not stored (they keep their bits whatever g holds)
//     else     :  update1 / average1 above with lr_over_bc1 * mu_g (one fp32 product) for lr_over_bc1 and decay_mul_g for decay_mul
// With mu == 1 everywhere and nothing frozen the stores are dcf_adamw_ema_step's bits (x * 1 = x).  Same two launch shapes; a wave of
// the flat shape reads 64 consecutive id bytes beside its one mask word.  An id is masked to the table's 16 entries and the entries from
// ngroups on are marked frozen, so an id the table does not hold stores nothing (ops.AdamGroups refuses such ids where they are built).
struct AdamGroupTable {
    float mu[DCF_ADAM_MAX_GROUPS], decay_mul[DCF_ADAM_MAX_GROUPS];
    uint32_t frozen;
};

namespace {

__device__ __forceinline__ bool group_scalars(AdamwScalars &cg, const AdamwScalars &c, const AdamGroupTable &t, const uint8_t *ids, int64_t group)
{
    const int id = ids[group] & (DCF_ADAM_MAX_GROUPS - 1);
    if ((t.frozen >> id) & 1u) return false;
    // the table sits in scalar registers (constant indices below): 2 x 15 selects per lane instead of two loads that depend on the
    // id load -- with the dependent loads the pass measured 2.2 us (1.8 %) over dcf_adamw_ema_step at the cfg2 arena size
    float mu = t.mu[0], dm = t.decay_mul[0];
#pragma unroll
    for (int k = 1; k < DCF_ADAM_MAX_GROUPS; ++k) {
        mu = id == k ? t.mu[k] : mu;
        dm = id == k ? t.decay_mul[k] : dm;
    }
    cg = c;
    cg.lr_over_bc1 = c.lr_over_bc1 * mu;
    cg.decay_mul = dm;
    return true;
}

template <bool EMA>
__device__ __forceinline__ void ggroup1(float *p, const float *g, float *m, float *v, float *e, const uint64_t *bits, const uint8_t *ids,
                                        int64_t n, int64_t group, const AdamwScalars &c, const AdamGroupTable &t)
{
    AdamwScalars cg;
    if (group_scalars(cg, c, t, ids, group)) group1<EMA>(p, g, m, v, e, bits, n, group, cg);
}

}  // namespace

template <bool GUARD, bool EMA>
__global__ void __launch_bounds__(kThreads) k_adamw_groups_flat(float *p, const float *g, float *m, float *v, float *e, const uint64_t *bits,
                                                                 const uint8_t *ids, int64_t n, AdamwScalars c, AdamGroupTable t,
                                                                 const dcf_amp_state *st)
{
    if (!scalars<GUARD>(c, st)) return;
    const int64_t group = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (group * 4 >= n) return;
    ggroup1<EMA>(p, g, m, v, e, bits, ids, n, group, c, t);
}

template <bool GUARD, bool EMA>
__global__ void __launch_bounds__(kThreads) k_adamw_groups_stride(float *p, const float *g, float *m, float *v, float *e, const uint64_t *bits,
                                                                   const uint8_t *ids, int64_t n, AdamwScalars c, AdamGroupTable t,
                                                                   const dcf_amp_state *st)
{
    if (!scalars<GUARD>(c, st)) return;
    const int64_t whole = n >> 2;
    const int64_t groups = (n + 3) >> 2;
    const int64_t step = (int64_t)gridDim.x * (2 * kThreads);
    int64_t base = (int64_t)blockIdx.x * (2 * kThreads);
    for (; base + 2 * kThreads <= whole; base += step) {      // both of the lane's groups whole; a frozen one loads nothing
        const int64_t ga = base + threadIdx.x, gb = ga + kThreads;
        const int64_t ia = ga * 4, ib = gb * 4;
        AdamwScalars ca, cb;
        const bool la = group_scalars(ca, c, t, ids, ga), lb = group_scalars(cb, c, t, ids, gb);
        float4 pa, ga4, ma, va, ea, pb, gb4, mb, vb, eb;
        if (la) {
            pa = ld4(p + ia); ga4 = ld4(g + ia); ma = ld4(m + ia); va = ld4(v + ia);
            if (EMA) ea = ld4(e + ia);
        }
        if (lb) {
            pb = ld4(p + ib); gb4 = ld4(g + ib); mb = ld4(m + ib); vb = ld4(v + ib);
            if (EMA) eb = ld4(e + ib);
        }
        if (la) {
            update4(pa, ga4, ma, va, decays(bits, ga), ca);
            st4(p + ia, pa); st4(m + ia, ma); st4(v + ia, va);
            if (EMA) st4(e + ia, average4(ea, pa, ca));
        }
        if (lb) {
            update4(pb, gb4, mb, vb, decays(bits, gb), cb);
            st4(p + ib, pb); st4(m + ib, mb); st4(v + ib, vb);
            if (EMA) st4(e + ib, average4(eb, pb, cb));
        }
    }
    if (base < groups) {                                  // the one chunk that is not whole (one workgroup gets here)
        const int64_t ga = base + threadIdx.x, gb = ga + kThreads;
        if (ga < groups) ggroup1<EMA>(p, g, m, v, e, bits, ids, n, ga, c, t);
        if (gb < groups) ggroup1<EMA>(p, g, m, v, e, bits, ids, n, gb, c, t);
    }
}

extern "C" int dcf_adamw_ema_step_groups(float *params, const float *grads, float *m, float *v, float *ema, const uint64_t *decay_bits,
                                         const uint8_t *group_ids, int ngroups, const dcf_adam_group *groups, int64_t n, float lr, float beta1,
                                         float beta2, float eps, int step, float gscale, float ema_omd, const dcf_amp_state *state,
                                         dcf_stream_t stream)
{
    DCF_REQUIRE(params && grads && m && v && group_ids && groups && n >= 0 && (state || step >= 1),
                "dcf_adamw_ema_step_groups: bad arguments (params %p, grads %p, m %p, v %p, group_ids %p, groups %p, n %lld, step %d, state %p)",
                (void *)params, (const void *)grads, (void *)m, (void *)v, (const void *)group_ids, (const void *)groups, (long long)n, step,
                (const void *)state);
    DCF_REQUIRE(ngroups >= 1 && ngroups <= DCF_ADAM_MAX_GROUPS, "dcf_adamw_ema_step_groups: 1 to %d groups (got %d)", DCF_ADAM_MAX_GROUPS, ngroups);
    DCF_REQUIRE(aligned(params, 16) && aligned(grads, 16) && aligned(m, 16) && aligned(v, 16) && aligned(ema, 16) && aligned(decay_bits, 8),
                "dcf_adamw_ema_step_groups: params, grads, m, v, ema must be 16-byte aligned and decay_bits 8-byte aligned");
    DCF_REQUIRE(isfinite(ema_omd) && ema_omd >= 0.f && ema_omd <= 1.f, "dcf_adamw_ema_step_groups: ema_omd must be in [0, 1] (got %g)", (double)ema_omd);
    DCF_REQUIRE(!ema || !(overlaps(ema, params, n) || overlaps(ema, grads, n) || overlaps(ema, m, n) || overlaps(ema, v, n)),
                "dcf_adamw_ema_step_groups: ema must not alias params, grads, m or v");
    AdamGroupTable t;
    t.frozen = 0xFFFFFFFFu;                               // an id past the table stores nothing
    for (int k = 0; k < DCF_ADAM_MAX_GROUPS; ++k) t.mu[k] = 0.f, t.decay_mul[k] = 1.f;
    for (int k = 0; k < ngroups; ++k) {
        DCF_REQUIRE(isfinite(groups[k].mu) && groups[k].mu >= 0.f && isfinite(groups[k].decay_mul),
                    "dcf_adamw_ema_step_groups: group %d: mu must be finite and not negative, decay_mul finite (got %g, %g)", k,
                    (double)groups[k].mu, (double)groups[k].decay_mul);
        t.mu[k] = groups[k].mu;
        t.decay_mul[k] = groups[k].decay_mul;
        if (!groups[k].frozen) t.frozen &= ~(1u << k);
    }
    if (n == 0) return DCF_OK;
    AdamwScalars c;
    c.b1 = beta1; c.b2 = beta2; c.eps = eps; c.decay_mul = 1.f; c.ema_omd = ema_omd;
    c.lr_over_bc1 = c.inv_sqrt_bc2 = c.gscale = 0.f;
    if (!state) {                                         // dcf_adam_step's host expressions
        const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
        c.lr_over_bc1 = (float)(lr / bc1);
        c.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
        c.gscale = gscale;
    }
    static DcfOpt shape_o("ADAMW_SHAPE");
    const char *shape = shape_o.str();
    const bool stride = shape ? strcmp(shape, "stride") == 0 : false;
    const int64_t ng4 = (n + 3) / 4;
    const int blocks = stride ? (int)(cdiv(ng4, 2 * kThreads) < kMaxBlocks ? cdiv(ng4, 2 * kThreads) : kMaxBlocks) : cdiv(ng4, kThreads);
    const double bytes = (double)n * (ema ? 36.0 : 28.0) + (double)n / 4.0 + (decay_bits ? (double)n / 32.0 : 0.0);
    hipStream_t s = S(stream);
#define DCF_ADAMW_G(GUARD_, EMA_)                                                                                                           \
    do {                                                                                                                                     \
        if (stride)                                                                                                                          \
            DCF_LAUNCH_B("adamw_ema_groups", bytes, s, hipLaunchKernelGGL((k_adamw_groups_stride<GUARD_, EMA_>), dim3(blocks), dim3(kThreads), 0, \
                                                                          s, params, grads, m, v, ema, decay_bits, group_ids, n, c, t, state)); \
        else                                                                                                                                 \
            DCF_LAUNCH_B("adamw_ema_groups", bytes, s, hipLaunchKernelGGL((k_adamw_groups_flat<GUARD_, EMA_>), dim3(blocks), dim3(kThreads), 0,  \
                                                                          s, params, grads, m, v, ema, decay_bits, group_ids, n, c, t, state)); \
    } while (0)
    if (state && ema) DCF_ADAMW_G(true, true);
    else if (state) DCF_ADAMW_G(true, false);
    else if (ema) DCF_ADAMW_G(false, true);
    else DCF_ADAMW_G(false, false);
#undef DCF_ADAMW_G
    return DCF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Gradient accumulation: dst = src (mode 0) or dst = dst + src (mode 1) over n floats, one fp32 add per
// element, no atomics -- every element has one writer.  Called on the whole gradient arena and on sub-ranges of it (the gradient
// buckets), so the pointers are only 4-byte aligned:
//     vec     dst and src share their offset modulo 16 bytes: `head` (0..3) elements up to the first 16-byte boundary go element by
//             element (lane t < head of the first workgroup takes element t), the rest is k_adamw_ema_flat's shape -- one float4 group
//             per lane, the ragged tail element by element
//     scalar  otherwise: one element per lane
// Both compute dst[i] + src[i] per element, so the result does not depend on the path.
template <int MODE>
__device__ __forceinline__ float accum1(float d, float s) { return MODE == 0 ? s : d + s; }

template <int MODE>
__global__ void __launch_bounds__(kThreads) k_grad_accum_vec(float *dst, const float *src, int64_t n, int head)
{
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t < head) dst[t] = accum1<MODE>(MODE == 0 ? 0.f : dst[t], src[t]);      // head <= n: the host clamps it
    const int64_t i4 = head + t * 4;
    if (i4 >= n) return;
    if (i4 + 4 <= n) {
        const float4 s = ld4(src + i4);
        float4 d = s;
        if (MODE != 0) {
            d = ld4(dst + i4);
            d.x = d.x + s.x; d.y = d.y + s.y; d.z = d.z + s.z; d.w = d.w + s.w;
        }
        st4(dst + i4, d);
    } else {
        for (int64_t i = i4; i < n; ++i) dst[i] = accum1<MODE>(MODE == 0 ? 0.f : dst[i], src[i]);
    }
}

template <int MODE>
__global__ void __launch_bounds__(kThreads) k_grad_accum_scalar(float *dst, const float *src, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) dst[i] = accum1<MODE>(MODE == 0 ? 0.f : dst[i], src[i]);
}

extern "C" int dcf_grad_accumulate(float *dst, const float *src, int64_t n, int mode, dcf_stream_t stream)
{
    DCF_REQUIRE(dst && src && n >= 0 && (mode == 0 || mode == 1), "dcf_grad_accumulate: bad arguments (dst %p, src %p, n %lld, mode %d)",
                (void *)dst, (const void *)src, (long long)n, mode);
    DCF_REQUIRE(aligned(dst, 4) && aligned(src, 4), "dcf_grad_accumulate: dst and src must be 4-byte aligned");
    DCF_REQUIRE(n <= ((int64_t)1 << 38), "dcf_grad_accumulate: n %lld is over the launch grid's range", (long long)n);
    DCF_REQUIRE(!overlaps(dst, src, n), "dcf_grad_accumulate: dst and src overlap");
    if (n == 0) return DCF_OK;
    const double bytes = (double)n * (mode == 0 ? 8.0 : 12.0);
    hipStream_t s = S(stream);
    if ((((uintptr_t)dst ^ (uintptr_t)src) & 15) == 0) {
        int64_t head = (int64_t)(((16 - ((uintptr_t)dst & 15)) & 15) / 4);
        if (head > n) head = n;
        int64_t lanes = (n - head + 3) / 4;
        if (lanes < head) lanes = head;
        const int blocks = cdiv(lanes, kThreads);
        if (mode == 0)
            DCF_LAUNCH_B("grad_accumulate", bytes, s, hipLaunchKernelGGL((k_grad_accum_vec<0>), dim3(blocks), dim3(kThreads), 0, s, dst, src, n, (int)head));
        else
            DCF_LAUNCH_B("grad_accumulate", bytes, s, hipLaunchKernelGGL((k_grad_accum_vec<1>), dim3(blocks), dim3(kThreads), 0, s, dst, src, n, (int)head));
    } else {
        const int blocks = cdiv(n, kThreads);
        if (mode == 0)
            DCF_LAUNCH_B("grad_accumulate", bytes, s, hipLaunchKernelGGL((k_grad_accum_scalar<0>), dim3(blocks), dim3(kThreads), 0, s, dst, src, n));
        else
            DCF_LAUNCH_B("grad_accumulate", bytes, s, hipLaunchKernelGGL((k_grad_accum_scalar<1>), dim3(blocks), dim3(kThreads), 0, s, dst, src, n));
    }
    return DCF_OK;
}
