"""The statements of tests/_bn_ref.py against F.batch_norm + autograd in fp64 on the CPU, their n = 1 closed form, the restated
walk, and the two facts the GPU bounds of tests/test_gpu_bn_edges.py rest on: a one-pass summation about a pivot, in the kernels'
own order and in fp32, stays inside every centred bound used there; the raw sums of x and x^2 in the same order do not."""
import pytest
import torch
import torch.nn.functional as F

import _bn_ref as R

DTYPES = ["f32", "bf16", "f16"]


def _close(got, want, what, rtol=1e-12):
    err = float((got - want).abs().max())
    assert err <= rtol * max(1.0, float(want.abs().max())), "%s: off by %.3g" % (what, err)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("momentum", [0.1, 1.0])
def test_statements_against_autograd(momentum, with_res, relu):
    npix, C, eps = 37, 12, 1e-3
    x = (R.normal((npix, C), 1) * 3 + 0.7).requires_grad_(True)
    gamma, beta = (R.normal((C,), 2) + 1.5).requires_grad_(True), R.normal((C,), 3).requires_grad_(True)
    res = R.normal((npix, C), 4) if with_res else None
    rm, rv = R.normal((C,), 5), R.normal((C,), 6).abs() + 0.5
    rm_t, rv_t = rm.clone(), rv.clone()
    y_t = F.batch_norm(x, rm_t, rv_t, gamma, beta, True, R.f32(momentum), R.f32(eps))
    if with_res:
        y_t = y_t + res
    if relu:
        y_t = torch.relu(y_t)
    mean, var, invstd, A, S1 = R.stats(x, eps)
    _close(A, ((x - x.mean(0)) ** 2).sum(0).detach(), "A")
    _close(S1, (x - x.mean(0)).abs().sum(0).detach(), "S1")
    y, n, Ay = R.apply_fwd(x, mean, invstd, gamma, beta, res, relu)
    _close(y, y_t.detach(), "y")
    assert n == 3 and bool((Ay >= y.abs() - 1e-12).all())
    new_m, new_v, bm, bv = R.running(rm, rv, mean, var, npix, momentum)
    _close(new_m, rm_t, "running_mean")
    _close(new_v, rv_t, "running_var")
    assert bool((bm >= 0).all()) and bool((bv > 0).all())
    g = R.normal((npix, C), 7)
    y_t.backward(g)
    g_in = g * (y > 0) if relu else g
    dbeta, dgamma, nn, Ab, Ag = R.bwd_sums(g_in, x, mean, invstd)
    _close(dbeta, beta.grad, "dbeta")
    _close(dgamma, gamma.grad, "dgamma")
    assert nn == npix and bool((Ab >= dbeta.abs() - 1e-12).all()) and bool((Ag >= dgamma.abs() - 1e-12).all())
    dx, n3, Ax = R.apply_bwd(g_in, x, mean, invstd, gamma, dgamma, dbeta, npix)
    _close(dx, x.grad, "dx")
    assert n3 == 3 and bool((Ax >= dx.abs() - 1e-12).all())


def test_one_pixel_closed_form():
    """n = 1: mean = x, var = 0, invstd = 1 / sqrt(eps), y = beta + res, the running variance takes var itself (0) for the
    unbiased one, dbeta = g, dgamma = 0, dx = 0."""
    C, eps, mom = 8, 1e-5, 0.1
    x, g, res = R.normal((1, C), 1) * 5, R.normal((1, C), 2), R.normal((1, C), 3)
    gamma, beta = R.normal((C,), 4) + 2, R.normal((C,), 5)
    rm, rv = R.normal((C,), 6), R.normal((C,), 7).abs() + 1
    mean, var, invstd, A, S1 = R.stats(x, eps)
    assert torch.equal(mean, x[0]) and not bool(var.any()) and not bool(A.any()) and not bool(S1.any())
    _close(invstd, torch.full((C,), R.f32(eps) ** -0.5, dtype=torch.float64), "invstd")
    y, _, _ = R.apply_fwd(x, mean, invstd, gamma, beta, res, False)
    _close(y, (beta + res), "y")
    new_m, new_v, _, _ = R.running(rm, rv, mean, var, 1, mom)
    _close(new_m, (1 - R.f32(mom)) * rm + R.f32(mom) * x[0], "running_mean")
    _close(new_v, (1 - R.f32(mom)) * rv, "running_var")
    dbeta, dgamma, _, _, _ = R.bwd_sums(g, x, mean, invstd)
    assert torch.equal(dbeta, g[0]) and not bool(dgamma.any())
    dx, _, _ = R.apply_bwd(g, x, mean, invstd, gamma, dgamma, dbeta, 1)
    assert not bool(dx.any())
    assert R.unbias(1) == 1.0 and R.unbias(5) == 1.25


def test_walk_restated():
    """bn_blocks() by hand: four vectors per thread, whole channel groups, at most BN_KTHREADS * 1024 threads."""
    assert R.walk(126, 96) == (8, 12, 1512, 372, 2)                  # test_bn_train_kernels' shape
    assert R.walk(4 * 131072 + 3, 8) == (8, 1, 524291, 131072, 512)  # the real cap: the workspace's 512 rows exactly
    assert R.chain_of(4 * 131072 + 3, 8) == 5 + 256
    assert R.walk(3, 1028) == (4, 257, 771, 257, 2) and R.walk(3, 2056) == (8, 257, 771, 257, 2)
    assert R.chain_of(3, 1028) == 3 + 1                              # more channel groups than threads in a workgroup
    assert R.walk(1, 4) == (4, 1, 1, 1, 1) and R.chain_of(1, 4) == 1 + 1
    assert R.walk(5000, 12, 1) == (4, 3, 15000, 1023, 4) and R.chain_of(5000, 12, 1) == 15 + 86
    assert R.chain_length(1512, 12) == 5 + 22
    assert R.walk(9, 64)[:4] == (8, 8, 72, 16)


def test_capped_walk_reaches_every_loop():
    """The census of the GPU test's capped sizes (host arithmetic only): over all threads, the four-in-flight body is taken once and
    twice, with tails of 0 .. 3, on one to four workgroups; its sizes under the default cap are the walks without the body."""
    for C in R.WALK_C:
        body, tail, blocks = set(), set(), set()
        for npix in R.capped_npix(C):
            V, cg, nvec, stride, nblk = R.walk(npix, C, 1)
            blocks.add(nblk)
            for t in range(stride):
                trips = len(range(t, nvec, stride))
                body.add(trips // 4)
                tail.add(trips % 4)
        assert body >= {1, 2} and tail == {0, 1, 2, 3} and blocks == {1, 2, 3, 4}, (C, body, tail, blocks)
        small = {len(range(0, R.walk(n, C)[2], R.walk(n, C)[3])) for n in R.SMALL_NPIX}
        assert small >= {1, 2, 3, 4}, (C, small)
    assert R.walk(2000, 12, 1)[3] % 256 != 0 and (256 % 3) != 0    # a partly idle last workgroup; workgroup 1 starts in group 1


def _stat_errors(x, eps, kthreads, pivot):
    npix, C = x.shape
    mean, var, _, _, _ = R.stats(x, eps)
    bm, bv = R.stats_bounds(x, eps, R.chain_of(npix, C, kthreads))
    em, ev = R.emulate_stats(x, eps, kthreads, pivot)
    return (em - mean).abs(), bm, (ev - var).abs(), bv


@pytest.mark.parametrize("dtype", DTYPES)
def test_pivot_order_meets_every_conditioning_bound(dtype):
    """Sums about a pivot, in the kernels' order and precision, stay inside the centred bounds on every conditioning case of the GPU
    test: the bounds ask for nothing a one-pass fp32 algorithm cannot give."""
    for npix, C, kthreads in R.CONDITIONING_SHAPES:
        x, ratio = R.conditioning_input(dtype, npix, C)
        assert {abs(float(r)) for r in ratio} == set(float(r) for r in R.RATIOS[dtype]) and bool((ratio < 0).any())
        em, bm, ev, bv = _stat_errors(x, 1e-5, kthreads, True)
        print("%s npix=%d C=%d: mean error / bound %.3g, var error / bound %.3g" % (dtype, npix, C, float((em / bm).max()), float((ev / bv).max())))
        assert bool((em <= bm).all()) and bool((ev <= bv).all())


def test_raw_sum_order_misses_the_bounds():
    """The raw sums of x and x^2 in the same order miss the variance bound on EVERY fp32 channel with |mean| / std >= 64: the GPU
    test can fail, and did on the kernels that summed so."""
    for npix, C, kthreads in R.CONDITIONING_SHAPES:
        x, ratio = R.conditioning_input("f32", npix, C)
        _, _, ev, bv = _stat_errors(x, 1e-5, kthreads, False)
        hard = ratio.abs() >= 64
        assert int(hard.sum()) >= 6
        assert bool((ev[hard] > bv[hard]).all()), "raw sums inside the bound at ratios %r" % ratio[hard][ev[hard] <= bv[hard]].tolist()
        assert bool((ev[ratio == 0] <= bv[ratio == 0]).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_pivot_order_on_the_special_channels(dtype):
    """Constant channels come out with var = 0 and mean = the constant exactly; the outlier and last-bit channels stay inside
    their bounds.  The raw sums give the constant 3.3 a variance."""
    for npix, kthreads in ((126, 128), (4096, 128), (4099, 1)):
        x = R.special_input(dtype, npix, 12)
        em, bm, ev, bv = _stat_errors(x, 1e-5, kthreads, True)
        assert not bool(bv[:4].any()) and not bool(ev[:4].any()) and not bool(em[:4].any())
        assert bool((em <= bm).all()) and bool((ev <= bv).all())
    _, raw_var = R.emulate_stats(R.special_input("f32", 4096, 12), 1e-5, 128, False)
    assert float(raw_var[1]) > 0


def test_special_input_is_what_it_says():
    for dtype in DTYPES:
        x = R.special_input(dtype, 126, 12).double()
        for c, v in enumerate(R.constant_values(dtype)):
            assert bool((x[:, c] == v).all())
        assert abs(R.constant_values(dtype)[3]) == R.FMAX[dtype] / 4
        assert int((x[:, 4] > 9000).sum()) == 1 and float(x[0, 4]) < 9000 and float(x[:, 4].abs().median()) < 2        # 1e4 is 9984 in bf16
        for c in (5, 6):
            vals = sorted(set(x[:, c].tolist()))
            assert len(vals) == 2
            lo, hi = torch.tensor(vals, dtype=torch.float64).to(R.TDT[dtype])
            assert abs(int(lo.view(torch.int32 if dtype == "f32" else torch.int16)) - int(hi.view(torch.int32 if dtype == "f32" else torch.int16))) == 1
