"""float64 statements of the train-mode BatchNorm kernels (csrc/elementwise.hip: k_bn_partial, k_bn_stats_final, k_bn_bwd_final,
k_bn_apply_fwd, k_bn_apply_bwd behind dcf_bn_train_fwd / dcf_bn_train_bwd), the inputs that put them at their edges, and a
restatement of the kernels' fp32 summation order in numpy (test infrastructure; CPU only: imports neither the GPU nor the library).

Every tensor is NHWC [npix, C], already rounded to the storage type; every statement evaluates it in fp64.  Every sum comes with
what tests/_fusion_ref.py::bound() needs: an fp32 sum of n terms with absolute sum A lies within 1.01 * (n + 8) * 2^-24 * A of the
fp64 value.  For the kernels' sums n is chain_length(): the longest chain of fp32 additions one partial goes through -- a thread's
trips plus the threads of one channel group in a workgroup; the workgroups' partials are added in double.

The statistics' bounds are on the CENTRED quantities: var within bound(chain, sum (x - mean)^2) / n and mean within
bound(chain, sum |x - mean|) / n + one fp32 ulp of |mean|, whatever |mean| / std is.  emulate_stats() shows on the CPU that a one-pass
algorithm meets them (sums about a pivot) and that raw sums of x and x^2 do not (tests/test_bn_ref_host.py).

The apply statements take the fp32 mean / invstd / dgamma / dbeta they are GIVEN, so the apply kernels are checked independently
of the sums."""
import numpy as np
import torch

from _fusion_ref import STORE_ULP, assert_within, bound          # noqa: F401  (re-exported: the tests take them from here)

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": 0, "bf16": 1, "f16": 2}                        # DCF_F32 / DCF_BF16 / DCF_F16
FMAX = {"f32": 3.4028234663852886e38, "bf16": 3.3895313892515355e38, "f16": 65504.0}
F32_EPS = 2.0 ** -24                                          # half an ulp, relative: one fp32 rounding
# |mean| / std of the conditioning cases: bf16 stops at 64 and fp16 at 512, where the stored values stop resolving the std
RATIOS = {"f32": (0, 8, 64, 512, 4096), "f16": (0, 8, 64, 512), "bf16": (0, 8, 64)}
SIGMAS = (1.0, 0.25, 4.0)


def f32(v):
    """The fp32 value nearest to v, as a Python float (what a c_float argument carries)."""
    return float(np.float32(v))


def _d(t):
    return t.detach().cpu().double()


# ---------------------------------------------------------------------------------------------------------------- the walk
def walk(npix, C, kthreads=128):
    """(V, cgroups, nvec, stride, nblk) of k_bn_partial's grid-stride walk: bn_blocks() of csrc/elementwise.hip restated, with
    BN_KTHREADS = kthreads (units of 1024 threads).  V channels per thread, `stride` threads of which each walks e, e + stride, ..."""
    V = 8 if C % 8 == 0 else 4
    cg = C // V
    nvec = npix * cg
    stride = _stride(nvec, cg, kthreads)
    return V, cg, nvec, stride, -(-stride // 256)


def _stride(nvec, cgroups, kthreads):
    # bn_blocks() of csrc/elementwise.hip: four vectors per thread, at most kthreads * 1024 threads, whole channel groups
    want = max(min((nvec + 3) // 4, kthreads * 1024), cgroups)
    return want // cgroups * cgroups


def chain_length(nvec, cgroups, kthreads=128):
    """The longest chain of fp32 additions behind one workgroup partial: the trips of one thread plus the threads of one channel
    group in a workgroup.  Restates bn_blocks() of csrc/elementwise.hip (through _stride()); the double finalisation adds nothing."""
    stride = _stride(nvec, cgroups, kthreads)
    trips = -(-nvec // stride)
    per_group = -(-min(256, stride) // cgroups)
    return trips + per_group


WALK_C = (4, 8, 12, 24, 64)                      # V = 4 and 8, channel groups 1, 1, 3, 3, 8
TRIPS = (1, 2, 3, 4, 5, 8, 9)                    # BN_KTHREADS = 1: nvec / stride just below, at and just above these
SMALL_NPIX = (1, 2, 3, 4, 5, 7, 8, 9)            # under the default cap


def capped_npix(C):
    """The pixel counts of the capped walk's cases: nvec / 1024 (1023 with three channel groups) around TRIPS."""
    V, cg, _, stride, _ = walk(10 ** 6, C, 1)
    assert stride == (1023 if cg == 3 else 1024)
    per = stride // cg                                           # pixels per trip of the whole capped grid
    return [k * per + d for k in TRIPS for d in (-1, 0, 1)]


def chain_of(npix, C, kthreads=128):
    V, cg, nvec, _, _ = walk(npix, C, kthreads)
    return chain_length(nvec, cg, kthreads)


# ---------------------------------------------------------------------------------------------------------------- statements
def stats(x, eps):
    """x [npix,C] -> (mean, biased var, invstd = 1 / sqrt(var + eps), A = sum (x - mean)^2, S1 = sum |x - mean|), each [C] fp64.
    eps is taken as the fp32 number the entry point receives.  A channel with an inf has mean +-inf and var, invstd NaN; one with
    a NaN has all three NaN."""
    x64 = _d(x)
    n = x64.shape[0]
    mean = x64.sum(0) / n
    dev = x64 - mean
    A = (dev * dev).sum(0)
    var = A / n
    return mean, var, 1.0 / torch.sqrt(var + f32(eps)), A, dev.abs().sum(0)


def stats_bounds(x, eps, chain):
    """(mean bound, var bound) [C] of the statistics of x: the centred bounds of the module's docstring."""
    mean, var, _, A, S1 = stats(x, eps)
    n = x.shape[0]
    zero = torch.zeros_like(mean)
    ulp = torch.from_numpy(np.spacing(np.abs(mean.numpy()).astype(np.float32)).astype(np.float64))
    return bound(chain, S1, zero) / n + ulp, bound(chain, A, zero) / n


def invstd_interval(var, var_bound, eps):
    """[lo, hi] of the fp32 invstd for a var within var_bound of `var`: the exact interval, widened by the one fp32 rounding of
    the store."""
    e = f32(eps)
    lo = 1.0 / torch.sqrt(var + var_bound + e)
    hi = 1.0 / torch.sqrt((var - var_bound).clamp(min=0.0) + e)
    return lo * (1 - F32_EPS), hi * (1 + F32_EPS)


def running(old_mean, old_var, mean, var, n, momentum):
    """The running statistics after one step -> (new mean, new var, bound of the mean's arithmetic, bound of the var's), fp64 [C].
    new = (1 - mom) * old + mom * batch with the UNBIASED batch variance var * n / (n - 1) -- for n = 1 var itself: that choice is
    the kernel's own (torch refuses n = 1 in training mode).  The kernel forms the update in fp32: 1 - mom, the cast of the batch
    value, the two products and the sum are three roundings on each of the two products, 3 * 2^-24 * (|(1 - mom) old| + |mom new|).
    The bounds do not include the error of mean / var themselves: the caller adds mom * (their bound)."""
    mom = f32(momentum)
    unb = var * n / (n - 1) if n > 1 else var
    om, ov = _d(old_mean), _d(old_var)
    t1m, t2m = (1 - mom) * om, mom * mean
    t1v, t2v = (1 - mom) * ov, mom * unb
    return t1m + t2m, t1v + t2v, 1.01 * 3 * F32_EPS * (t1m.abs() + t2m.abs()), 1.01 * 3 * F32_EPS * (t1v.abs() + t2v.abs())


def unbias(n):
    return n / (n - 1.0) if n > 1 else 1.0


def apply_fwd(x, mean32, invstd32, gamma, beta, res, relu):
    """y = act((x - mean) * invstd * gamma + beta + res) from the fp32 mean / invstd GIVEN -> (y fp64 [npix,C], n = 3,
    A = |(x - mean) invstd gamma| + |beta| + |res| per element).  The ReLU is 1-Lipschitz: the bound of its argument holds after it."""
    t = (_d(x) - _d(mean32)) * _d(invstd32) * _d(gamma)
    y, A = t + _d(beta), t.abs() + _d(beta).abs()
    if res is not None:
        y, A = y + _d(res), A + _d(res).abs()
    return (torch.relu(y) if relu else y), 3, A


def bwd_sums(g, x, mean32, invstd32):
    """dbeta = sum g, dgamma = sum g * xhat with xhat = (x - mean) * invstd from the fp32 statistics GIVEN ->
    (dbeta, dgamma, n = npix, A_dbeta = sum |g|, A_dgamma = sum |g xhat|), fp64 [C]."""
    g64 = _d(g)
    t = g64 * ((_d(x) - _d(mean32)) * _d(invstd32))
    return g64.sum(0), t.sum(0), g64.shape[0], g64.abs().sum(0), t.abs().sum(0)


def apply_bwd(g, x, mean32, invstd32, gamma, dgamma32, dbeta32, n):
    """dx = gamma * invstd * (g - dbeta / n - xhat * dgamma / n) from the fp32 statistics and sums GIVEN -> (dx fp64, n = 3,
    A = |gamma invstd| * (|g| + |dbeta / n| + |xhat dgamma / n|) per element)."""
    g64, k = _d(g), _d(gamma) * _d(invstd32)
    xh = (_d(x) - _d(mean32)) * _d(invstd32)
    tb, tg = _d(dbeta32) / n, xh * _d(dgamma32) / n
    dx, A = k * (g64 - tb - tg), k.abs() * (g64.abs() + tb.abs() + tg.abs())
    # an exact zero (one pixel; the third pixel where two of three are equal) comes out of fp64 as 1e-16 of A: stated as zero, at
    # 1e-9 of A far inside the bound's 11 * 2^-24 of it
    return torch.where(dx.abs() <= 1e-9 * A, torch.zeros_like(dx), dx), 3, A


# ---------------------------------------------------------------------------------------------------------------- the kernel's order
def emulate_stats(x, eps, kthreads=128, pivot=True):
    """(mean, var) fp64 [C] as k_bn_partial<T, false, V> + k_bn_stats_final form them, restated in numpy: every thread adds its
    elements trip by trip in fp32 (d = x - p, s += d, q += d * d: separate roundings, the library is built without contraction),
    one thread per output adds the workgroup's threads of its channel group in thread order in fp32, the workgroups' partials are
    added in double.  pivot=True: p = the channel's first pixel (0 where that is not finite), mean = p + s / n,
    var = q / n - (s / n)^2.  pivot=False: p = 0, the raw sums of x and x^2."""
    a = x.detach().cpu().float().numpy()
    npix, C = a.shape
    V, cg, nvec, stride, nblk = walk(npix, C, kthreads)
    m = stride // cg                                              # threads per channel group; pixel p: thread p % m, trip p // m
    with np.errstate(all="ignore"):
        p = np.where(np.abs(a[0]) <= np.float32(3.402823466e38), a[0], np.float32(0)) if pivot else np.zeros(C, np.float32)
        d = a - p
        assert d.dtype == np.float32
        s, q = np.zeros((m, C), np.float32), np.zeros((m, C), np.float32)
        for k in range(-(-npix // m)):
            rows = d[k * m:(k + 1) * m]
            s[:len(rows)] += rows
            q[:len(rows)] += rows * rows
        # thread u of channel group j is global thread u * cg + j: workgroup (u * cg + j) // 256
        grp = np.arange(C) // V
        ps, pq = np.zeros((nblk, C), np.float32), np.zeros((nblk, C), np.float32)
        cols = np.arange(C)
        for u in range(m):
            blk = (u * cg + grp) // 256
            ps[blk, cols] += s[u]
            pq[blk, cols] += q[u]
        assert ps.dtype == np.float32 and pq.dtype == np.float32
        off = ps.astype(np.float64).sum(0) / npix
        var = np.maximum(pq.astype(np.float64).sum(0) / npix - off * off, 0.0)
        return torch.from_numpy(p.astype(np.float64) + off), torch.from_numpy(var)


# ---------------------------------------------------------------------------------------------------------------- inputs
def normal(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def conditioning_input(dtype, npix, C, seed=0):
    """x [npix,C] of the storage type: channel c is mu + sigma * N(0,1) with |mu| / sigma running through RATIOS[dtype], both signs
    of mu and three sigmas, so that neighbouring channels differ in ratio, sign and scale.  Returns (x, ratio per channel)."""
    ratios = RATIOS[dtype]
    z = normal((npix, C), 100 + seed)
    ratio = torch.tensor([ratios[(c // 2) % len(ratios)] * (1.0 if c % 2 == 0 else -1.0) for c in range(C)], dtype=torch.float64)
    sigma = torch.tensor([SIGMAS[c % 3] for c in range(C)], dtype=torch.float64)
    x = ((ratio + z) * sigma).to(TDT[dtype])
    assert bool(torch.isfinite(x.float()).all())
    return x, ratio


CONDITIONING_SHAPES = ((126, 12, 128), (509, 16, 128), (4096, 12, 128), (4099, 24, 1))      # (npix, C, BN_KTHREADS)


def constant_values(dtype):
    """The constants of the constant-channel cases, as values of the storage type."""
    return [float(torch.tensor(v, dtype=torch.float64).to(TDT[dtype]).double()) for v in (0.0, 3.3, -1e4, FMAX[dtype] / 4)]


def special_input(dtype, npix, C, seed=0):
    """x [npix,C] of the storage type, N(0,1) except: channels 0-3 constant (constant_values), channel 4 one outlier of 1e4 (not at
    the first pixel, which the kernel takes as its pivot), channel 5 two adjacent values of the type around 3 (they differ in the last
    bit), channel 6 the same around -1000."""
    td = TDT[dtype]
    x = normal((npix, C), 200 + seed).to(td)
    for c, v in enumerate(constant_values(dtype)):
        x[:, c] = v
    if npix > 1:
        x[npix // 2, 4] = 1e4
    pick = (torch.arange(npix) * 7 % 3 == 0)
    for c, base in ((5, 3.0), (6, -1000.0)):
        lo = torch.tensor(base, dtype=td)
        hi = torch.nextafter(lo.float(), torch.tensor(float("inf"))).to(td) if td == torch.float32 else _next_up(lo)
        assert float(hi) != float(lo)
        x[:, c] = torch.where(pick, hi, lo)
    return x


def _next_up(t):
    """The next value of a 16-bit type towards +inf."""
    b = t.view(torch.int16)
    return (b + (1 if float(t) >= 0 else -1)).view(t.dtype)


def repair_subnormal(make_want, t, step, dtype, tries=32):
    """For fp16 results: `t` [npix,C] (storage type) with step added (even rows) or subtracted (odd rows), and rounded again, wherever make_want(t) has a non-zero element below
    2^-13 -- twice the smallest normal fp16 number, so that a result formed from slightly different fp32 statistics stays normal.
    Other types: t as it is."""
    if dtype != "f16":
        return t
    for _ in range(tries):
        w = make_want(t)
        bad = (w != 0) & (w.abs() < 2.0 ** -13)
        if not bool(bad.any()):
            return t
        sign = (1 - 2 * (torch.arange(t.shape[0]) % 2)).double().reshape(-1, 1)      # by row: two bad rows of a channel move apart
        t = torch.where(bad, (t.double() + step * sign).to(t.dtype), t)
        if _ >= 8:
            step *= 2           # a result that hardly depends on t (dx of the odd pixel out of three, through eps alone) wants a large move
    raise AssertionError("repair_subnormal: results in the subnormal range after %d passes" % tries)
