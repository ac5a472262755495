"""The train-mode BatchNorm kernels (csrc/elementwise.hip: k_bn_partial, k_bn_stats_final, k_bn_bwd_final, k_bn_apply_fwd,
k_bn_apply_bwd) through the two C-ABI entry points, against the fp64 statements of tests/_bn_ref.py at the smallest shapes at which
they can still go wrong.

No bound here is a bare tolerance.  The statistics: var within bound(chain, sum (x - mean)^2) / n and mean within
bound(chain, sum |x - mean|) / n + one fp32 ulp -- the CENTRED energy, whatever |mean| / std (tests/test_bn_ref_host.py shows that a
one-pass fp32 summation meets them and that raw sums of x and x^2 do not); invstd inside the exact image of the var interval; the
running statistics within R.running()'s three fp32 roundings on top.  dgamma / dbeta: bound(chain, A) with A from the statement.
y and dx: the statement evaluated with the fp32 statistics and sums the kernels RETURNED, bound(3, A) plus the storage rounding,
so the apply kernels are checked independently of the sums.  chain is R.chain_length(): trips of a thread plus threads of a channel
group in a workgroup.

The walk has up to 128 k threads, four vectors each; BN_KTHREADS = 1 caps it at 1024 threads, so that tensors of a few thousand
vectors reach the four-in-flight body more than once, its tail, a last workgroup with idle threads and workgroups whose first thread
is not in channel group 0.  Every output tensor is followed by guard rows that must keep their pattern, the workspace by guard
bytes.  fp16: the storage term of the bound is relative, so the inputs are repaired until every stored result is zero or normal."""
import pytest
import torch

import _bn_ref as R
from _elementwise_ref import bits, same_bits
from _util import pkg

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
GUARD_ROWS, GUARD_BYTES, GUARD_VALUE, INIT = 3, 4096, -7.0, 0.25


@pytest.fixture
def set_opt():
    """H.set_option for the test's duration: every option set is back to None afterwards."""
    H = pkg("_hip")
    names = []

    def f(name, value):
        names.append(name)
        H.set_option(name, value)
    yield f
    for n in names:
        H.set_option(n, None)


def _workspace(C):
    nbytes = int(pkg("_hip").lib().dcf_bn_workspace_bytes(C))
    ws = torch.full((nbytes + GUARD_BYTES,), 0xA5, dtype=torch.uint8, device="cuda")
    return ws, nbytes


def _guarded(npix, C, td):
    return torch.full((npix + GUARD_ROWS, C), GUARD_VALUE, dtype=td, device="cuda")


def _guard_intact(buf, npix, what):
    assert bool((buf[npix:].float() == GUARD_VALUE).all()), what + ": wrote past the tensor's end"


def _ws_intact(ws, nbytes, what):
    assert bool((ws[nbytes:] == 0xA5).all()), what + ": wrote past the workspace's end"


def run_fwd(dtype, x, gamma, beta, res, rm, rv, relu, eps, momentum):
    """dcf_bn_train_fwd on guarded buffers -> dict of CPU results (y in the storage type, the rest fp32)."""
    H, td = pkg("_hip"), R.TDT[dtype]
    npix, C = x.shape
    ws, nbytes = _workspace(C)
    y = _guarded(npix, C, td)
    mean, invstd = [torch.full((C,), float("nan"), device="cuda") for _ in range(2)]
    rmd = None if rm is None else rm.float().cuda()
    rvd = None if rv is None else rv.float().cuda()
    xd = x.cuda()
    H.call("dcf_bn_train_fwd", R.CODE[dtype], xd, gamma.float().cuda(), beta.float().cuda(), None if res is None else res.cuda(), y,
           mean, invstd, rmd, rvd, npix, C, eps, momentum, int(relu), ws, H.stream_ptr())
    torch.cuda.synchronize()
    what = "bn_train_fwd %s npix=%d C=%d" % (dtype, npix, C)
    _guard_intact(y, npix, what)
    _ws_intact(ws, nbytes, what)
    assert torch.equal(bits(xd), bits(x)), what + " wrote x"
    return dict(y=y[:npix].cpu(), mean=mean.cpu(), invstd=invstd.cpu(), rm=None if rm is None else rmd.cpu(), rv=None if rv is None else rvd.cpu())


def run_bwd(dtype, g, x, mean32, invstd32, gamma):
    """dcf_bn_train_bwd on guarded buffers; dgamma / dbeta hold INIT on entry (the call overwrites them)."""
    H, td = pkg("_hip"), R.TDT[dtype]
    npix, C = x.shape
    ws, nbytes = _workspace(C)
    dx = _guarded(npix, C, td)
    dgamma, dbeta = [torch.full((C,), INIT, device="cuda") for _ in range(2)]
    H.call("dcf_bn_train_bwd", R.CODE[dtype], g.cuda(), x.cuda(), mean32.cuda(), invstd32.cuda(), gamma.float().cuda(), dgamma, dbeta, dx,
           npix, C, ws, H.stream_ptr())
    torch.cuda.synchronize()
    what = "bn_train_bwd %s npix=%d C=%d" % (dtype, npix, C)
    _guard_intact(dx, npix, what)
    _ws_intact(ws, nbytes, what)
    return dict(dx=dx[:npix].cpu(), dgamma=dgamma.cpu(), dbeta=dbeta.cpu())


def _within(got, want, allowed, what):
    got = got.double()
    assert bool(torch.isfinite(got).all()), "%s: %d non-finite elements" % (what, int((~torch.isfinite(got)).sum()))
    over = (got - want).abs() - allowed
    i = int(over.argmax())
    print("%s: max |got - want| %.3g, largest excess over the bound %.3g" % (what, float((got - want).abs().max()), float(over.max())))
    assert float(over.max()) <= 0, "%s: channel %d got %.9g want %.9g, %.3g beyond the bound %.3g; %d channels beyond it" % (
        what, i, float(got[i]), float(want[i]), float(over[i]), float(allowed[i]), int((over > 0).sum()))


def check_stats(what, out, x, eps, momentum, rm0, rv0, kthreads, good=None):
    """mean, invstd and the running statistics of `out` against the statements, on the channels of `good` (default: all)."""
    npix, C = x.shape
    good = torch.ones(C, dtype=torch.bool) if good is None else good
    chain = R.chain_of(npix, C, kthreads)
    mean, var, invstd, _, _ = R.stats(x[:, good], eps)
    bm, bv = R.stats_bounds(x[:, good], eps, chain)
    _within(out["mean"][good], mean, bm, what + " mean")
    lo, hi = R.invstd_interval(var, bv, eps)
    got = out["invstd"][good].double()
    assert bool(torch.isfinite(got).all()), what + " invstd: non-finite"
    over = torch.maximum(lo - got, got - hi)
    print("%s invstd: largest excess over its interval %.3g (relative width %.3g)" % (what, float(over.max()), float(((hi - lo) / lo).max())))
    assert float(over.max()) <= 0, "%s invstd: channel %d got %.9g outside [%.9g, %.9g]; var %.6g +- %.3g" % (
        what, int(over.argmax()), float(got[over.argmax()]), float(lo[over.argmax()]), float(hi[over.argmax()]),
        float(var[over.argmax()]), float(bv[over.argmax()]))
    if rm0 is not None:
        mom = R.f32(momentum)
        new_m, new_v, am, av = R.running(rm0[good], rv0[good], mean, var, npix, momentum)
        _within(out["rm"][good], new_m, am + mom * bm, what + " running_mean")
        _within(out["rv"][good], new_v, av + mom * R.unbias(npix) * bv, what + " running_var")
    else:
        assert out["rm"] is None and out["rv"] is None


def check_apply_fwd(what, dtype, out, x, gamma, beta, res, relu, good=None):
    want, n, A = R.apply_fwd(x, out["mean"], out["invstd"], gamma.float(), beta.float(), res, relu)
    y = out["y"]
    if good is not None:
        want, A, y = want[:, good], A[:, good], y[:, good]
    R.assert_within(y, want, n, A, R.TDT[dtype], what + " y")


def check_bwd(what, dtype, outb, g, x, mean32, invstd32, gamma, kthreads):
    npix, C = x.shape
    chain = R.chain_of(npix, C, kthreads)
    dbeta, dgamma, n, Ab, Ag = R.bwd_sums(g, x, mean32, invstd32)
    assert n == npix
    R.assert_within(outb["dbeta"], dbeta, chain, Ab, torch.float32, what + " dbeta")
    R.assert_within(outb["dgamma"], dgamma, chain, Ag, torch.float32, what + " dgamma")
    want, n3, A = R.apply_bwd(g, x, mean32, invstd32, gamma.float(), outb["dgamma"], outb["dbeta"], npix)
    R.assert_within(outb["dx"], want, n3, A, R.TDT[dtype], what + " dx")


def make_case(dtype, npix, C, seed, with_res=True, relu=True, eps=1e-5, x=None):
    """Inputs of one case on the CPU: x, res, g in the storage type (fp16: repaired so that y and dx are zero or normal), fp32
    gamma, beta and running statistics."""
    td = R.TDT[dtype]
    if x is None:
        x = (R.normal((npix, C), seed) * 1.5 + 0.5).to(td)
    gamma = (R.normal((C,), seed + 1) * 0.3 + 1.2).float()
    beta = (R.normal((C,), seed + 2) * 0.5).float()
    res = R.normal((npix, C), seed + 3).to(td) if with_res else None
    # fp16: dx scaled away from the subnormal range; two pixels leave of g only the part eps / (var + eps) of its deviation
    g_scale = 1.0 if dtype != "f16" else 2048.0 if npix == 2 else 8.0
    g = (R.normal((npix, C), seed + 4) * g_scale).to(td)
    g[3::5] = 0                                                 # what a ReLU mask upstream leaves
    rm, rv = R.normal((C,), seed + 5).float(), (R.normal((C,), seed + 6).abs() + 0.5).float()

    def y_of(xx, rr):
        m, _, i, _, _ = R.stats(xx, eps)
        return R.apply_fwd(xx, m, i, gamma, beta, rr, relu)[0]
    if with_res:
        res = R.repair_subnormal(lambda r: y_of(x, r), res, 2.0 ** -6, dtype)
    else:
        x = R.repair_subnormal(lambda t: y_of(t, None), x, 2.0 ** -4, dtype)

    def dx_of(gg):
        m, _, i, _, _ = R.stats(x, eps)
        db, dg, _, _, _ = R.bwd_sums(gg, x, m, i)
        return R.apply_bwd(gg, x, m, i, gamma, dg, db, npix)[0]
    if npix > 1:                                                # one pixel: dx is zero whatever g
        g = R.repair_subnormal(dx_of, g, g_scale / 32, dtype)
    return dict(x=x, gamma=gamma, beta=beta, res=res, g=g, rm=rm, rv=rv, relu=relu, eps=eps)


def full_check(what, dtype, c, kthreads=128, momentum=0.1, running=True, good=None, backward=True):
    """Forward and backward of one case against every statement; returns the two result dicts."""
    rm, rv = (c["rm"], c["rv"]) if running else (None, None)
    out = run_fwd(dtype, c["x"], c["gamma"], c["beta"], c["res"], rm, rv, c["relu"], c["eps"], momentum)
    check_stats(what, out, c["x"], c["eps"], momentum, rm, rv, kthreads, good)
    check_apply_fwd(what, dtype, out, c["x"], c["gamma"], c["beta"], c["res"], c["relu"], good)
    if not backward:
        return out, None
    outb = run_bwd(dtype, c["g"], c["x"], out["mean"], out["invstd"], c["gamma"])
    check_bwd(what, dtype, outb, c["g"], c["x"], out["mean"], out["invstd"], c["gamma"], kthreads)
    return out, outb


# ------------------------------------------------------------------------------------------------------------------ walk and layout
@pytest.mark.parametrize("C", R.WALK_C)
@pytest.mark.parametrize("dtype", DTYPES)
def test_walk_default_cap(dtype, C):
    """npix 1 .. 9: fewer vectors than four per thread, one thread, a single trip and its tail."""
    for npix in R.SMALL_NPIX:
        full_check("default cap %s C=%d npix=%d" % (dtype, C, npix), dtype, make_case(dtype, npix, C, 10 * npix + C))


@pytest.mark.parametrize("C", R.WALK_C)
@pytest.mark.parametrize("dtype", DTYPES)
def test_walk_capped(dtype, C, set_opt):
    """BN_KTHREADS = 1: nvec / 1024 just below, at and just above 1, 2, 3, 4, 5, 8, 9 -- up to four vectors per thread the grid
    grows with the tensor (one to four workgroups), beyond that the threads walk: the four-in-flight body once and twice, every
    length of its tail, the last workgroup partly idle (C = 12, 24: 1023 threads), first threads outside channel group 0."""
    set_opt("BN_KTHREADS", 1)
    for npix in R.capped_npix(C):
        full_check("capped %s C=%d npix=%d" % (dtype, C, npix), dtype, make_case(dtype, npix, C, npix % 97 + C), kthreads=1)


@pytest.mark.parametrize("C", (1028, 2056))
@pytest.mark.parametrize("dtype", DTYPES)
def test_more_channel_groups_than_threads(dtype, C):
    """257 channel groups: a workgroup of 256 threads holds no thread of one of them."""
    assert R.walk(3, C)[1] == 257
    full_check("cg=257 %s C=%d" % (dtype, C), dtype, make_case(dtype, 3, C, C))


def test_real_cap_fills_the_workspace():
    """C = 8, npix = 4 * 131072 + 3 (fp32): 512 workgroups, the workspace exactly full, a fifth trip for three threads."""
    npix, C = 4 * 131072 + 3, 8
    assert R.walk(npix, C)[3:] == (131072, 512)
    assert int(pkg("_hip").lib().dcf_bn_workspace_bytes(C)) == 4 * 2 * C * 512
    c = make_case("f32", npix, C, 5)
    full_check("real cap", "f32", c)


# ------------------------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("shape", R.CONDITIONING_SHAPES, ids=["%dx%d_k%d" % s for s in R.CONDITIONING_SHAPES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_conditioning(dtype, shape, set_opt):
    """x = mu + sigma N(0,1) with |mu| / sigma up to 4096 (fp32), 512 (fp16), 64 (bf16), both signs, three sigmas in one tensor:
    var within the bound of the CENTRED energy."""
    npix, C, kthreads = shape
    set_opt("BN_KTHREADS", None if kthreads == 128 else kthreads)
    x, ratio = R.conditioning_input(dtype, npix, C)
    for momentum, eps in ((0.1, 1e-5), (1.0, 1e-3)):
        c = make_case(dtype, npix, C, 3, eps=eps, x=x)
        full_check("conditioning %s %r mom=%g eps=%g" % (dtype, shape, momentum, eps), dtype, c, kthreads=kthreads, momentum=momentum)


@pytest.mark.parametrize("npix_k", ((126, 128), (4096, 128), (4099, 1)), ids=["126", "4096", "4099_k1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_channels(dtype, npix_k, set_opt):
    """Constant channels (0, 3.3, -1e4, the largest finite value / 4): var = 0 exactly, so invstd = 1 / sqrt(eps) rounded to fp32,
    mean the constant and y = beta + res bit for bit; one outlier of 1e4; channels whose values differ in the last bit only."""
    npix, kthreads = npix_k
    set_opt("BN_KTHREADS", None if kthreads == 128 else kthreads)
    C, eps, td = 12, 1e-5, R.TDT[dtype]
    c = make_case(dtype, npix, C, 7, relu=False, eps=eps, x=R.special_input(dtype, npix, C))
    out, _ = full_check("special %s npix=%d" % (dtype, npix), dtype, c, kthreads=kthreads)
    consts = torch.tensor(R.constant_values(dtype), dtype=torch.float64)
    want_invstd = torch.tensor(R.f32(eps), dtype=torch.float64).rsqrt().float()
    assert torch.equal(out["invstd"][:4], want_invstd.expand(4)), "constant channels: invstd %r, want %r" % (out["invstd"][:4].tolist(), float(want_invstd))
    assert torch.equal(out["mean"][:4].double(), consts), "constant channels: mean %r" % out["mean"][:4].tolist()
    same_bits(out["y"][:, :4], (c["beta"][:4] + c["res"][:, :4].float()).to(td), "constant channels: y = beta + res")


@pytest.mark.parametrize("where", ("first", "middle"))
@pytest.mark.parametrize("kind", ("nan", "inf"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_containment(dtype, kind, where):
    """One NaN / one +inf in ONE channel (at the first pixel -- the kernel's pivot -- and elsewhere): that channel's statistics and y
    are non-finite as the statement says (mean NaN / +inf, invstd NaN, y NaN); every other channel, running statistics included,
    stays within its bound."""
    npix, C, bad = 126, 12, 5
    c = make_case(dtype, npix, C, 11)
    x = c["x"].clone()
    x[0 if where == "first" else 77, bad] = float(kind)
    c["x"] = x
    good = torch.arange(C) != bad
    out, _ = full_check("containment %s %s %s" % (dtype, kind, where), dtype, c, good=good, backward=False)
    mean, var, invstd, _, _ = R.stats(x, c["eps"])
    assert torch.isnan(invstd[bad]) and torch.isnan(var[bad]) and (torch.isnan(mean[bad]) if kind == "nan" else float(mean[bad]) == float("inf"))
    same_bits(out["mean"][bad], mean[bad].float(), "the bad channel's mean")
    assert torch.isnan(out["invstd"][bad]) and bool(torch.isnan(out["y"][:, bad].float()).all())
    assert not bool(torch.isfinite(out["rm"][bad])) and not bool(torch.isfinite(out["rv"][bad]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_pixel(dtype):
    """n = 1: var = 0, the running variance takes the biased variance (0) for the unbiased one, dx = 0, dgamma = 0, dbeta = g."""
    for C in (4, 8, 24):
        c = make_case(dtype, 1, C, 13 + C)
        out, outb = full_check("one pixel %s C=%d" % (dtype, C), dtype, c)
        assert torch.equal(out["mean"], c["x"][0].float())
        assert torch.equal(out["rv"].double(), ((1 - torch.tensor(R.f32(0.1)).float()) * c["rv"]).double())
        assert not bool(outb["dx"].float().any()) and not bool(outb["dgamma"].any()) and torch.equal(outb["dbeta"], c["g"][0].float())


# ------------------------------------------------------------------------------------------------------------------ apply kernels
@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("with_res", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_variants(dtype, with_res, relu, set_opt):
    """res in {None, tensor} x relu in {0, 1}, with and without running statistics, V = 4 and 8; y and dx from the kernels' own
    returned statistics and sums, guard rows behind both, dgamma / dbeta overwritten (they held 0.25)."""
    set_opt("BN_KTHREADS", 1)
    for C, npix, running in ((12, 1370, True), (16, 701, False)):
        c = make_case(dtype, npix, C, 17 + C, with_res=with_res, relu=relu)
        out, _ = full_check("apply %s C=%d res=%d relu=%d" % (dtype, C, with_res, relu), dtype, c, kthreads=1, running=running)
        if relu:
            zeros = float((out["y"].float() == 0).float().mean())
            assert 0.05 < zeros < 0.95, "the ReLU clips %.2f of y" % zeros


# ------------------------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("dtype", DTYPES)
def test_twice_the_same_bits(dtype, set_opt):
    """Forward and backward run twice give identical bits in every output (no float atomics in the sums)."""
    for kthreads, npix, C in ((1, 2731, 24), (128, 4099, 16)):
        set_opt("BN_KTHREADS", None if kthreads == 128 else kthreads)
        c = make_case(dtype, npix, C, 23)
        runs = []
        for _ in range(2):
            out = run_fwd(dtype, c["x"], c["gamma"], c["beta"], c["res"], c["rm"], c["rv"], True, 1e-5, 0.1)
            outb = run_bwd(dtype, c["g"], c["x"], out["mean"], out["invstd"], c["gamma"])
            runs.append({**out, **outb})
        for k in runs[0]:
            assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), "%s differs between two runs" % k
