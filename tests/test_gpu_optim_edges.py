"""GPU suite: the optimiser-step kernels against the fp32 statements of tests/_optim_ref.py (checked on the CPU by
tests/test_optim_ref_host.py) -- k_adam, k_adam_guarded and k_adamw_ema flat / stride bit for bit at every size that crosses a lane
group, a workgroup or a chunk, with zero, negative-zero, denormal, overflowing and non-finite values planted and from zero and
non-zero moments; k_grad_stats counting every element exactly once and flagging every position; k_amp_update's single-lane branches
field by field; FlatAdam.step's four branches on a stub model.  Every array handed to a kernel is a 16-byte-aligned view with 8
canary floats in front and behind, unchanged after every launch.  Comparison rule: a NaN equals a NaN, everything else by bits."""
import numpy as np
import pytest
import torch

import _optim_ref as R
from _util import pkg

pytestmark = pytest.mark.gpu

F = np.float32
LR, B1, B2 = R.LR, R.B1, R.B2
CANARY = -1234567.0
GUARD = 8
# (non-zero start moments, gscale, eps): eps = 0 makes the quotient 0 / 0 = NaN wherever v' = 0, on both sides
COMBOS = [(nz, gs, eps) for nz in (False, True) for gs in (0.37, 1.0) for eps in (1e-8, 0.0)]
S = R.STRIDE
DM = R.DECAY_MUL                      # float32(1 - 1e-3 * 0.01)


class Guarded(object):
    """A device array as a view into a larger buffer: GUARD canary elements in front (so the view starts 32 bytes into the
    allocation: 16-byte aligned) and behind."""

    def __init__(self, data, canary=CANARY, dtype=torch.float32):
        n = len(data)
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + n]
        if n:
            self.view.copy_(data if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data)))
        assert self.view.data_ptr() % 16 == 0
        self.edges = self._edges().clone()

    def _edges(self):
        e = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]])
        return e.view(torch.int32) if e.dtype == torch.float32 else e

    def intact(self):
        return torch.equal(self._edges(), self.edges)

    def set(self, data):
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(data)))

    def get(self):
        return self.view.cpu().numpy()


def _mask(kind, n, seed=0):
    words = R.mask_words(kind, n, seed)
    if words is None:
        return None, None
    return words, Guarded(words.view(np.int64), 0x5A5A5A5A5A5A5A5A, torch.int64)


def _same(got, want, what):
    ok = R.same_bits(got, want)
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        raise AssertionError("%s: %d of %d elements differ, first at %d: got %r (0x%08x), want %r (0x%08x)" % (
            what, int((~ok).sum()), len(ok), i, got[i], int(np.asarray(got[i:i + 1], dtype=F).view(np.uint32)[0]), want[i],
            int(np.asarray(want[i:i + 1], dtype=F).view(np.uint32)[0])))


def _intact(arrays, what):
    for k, a in enumerate(arrays):
        assert a is None or a.intact(), "%s: canaries of array %d changed" % (what, k)


@pytest.fixture(params=["flat", "stride"])
def shape(request):
    H = pkg("_hip")
    H.set_option("ADAMW_SHAPE", request.param)
    yield request.param
    H.set_option("ADAMW_SHAPE", None)


_CLEAN = None


def _clean_state(ops, st, gscale_host, t):
    """The state of applied step t from the real dcf_grad_stats + dcf_amp_update on a clean gradient (scale 1, no clipping); returns
    (lr_over_bc1, inv_sqrt_bc2, gscale) read back from it."""
    global _CLEAN
    if _CLEAN is None:
        _CLEAN = Guarded(np.array([3.0, 4.0, 0.0, 0.0, 1.0], dtype=F))
    st.applied_steps.fill_(t - 1)
    ops.grad_stats(_CLEAN.view, st)
    ops.amp_update(st, gscale_host, False, 2.0, 0.5, 2000, None, LR, B1, B2)
    h = _header(st)
    assert h.found_inf == 0 and h.applied_steps == t and _CLEAN.intact()
    return F(h.lr_over_bc1), F(h.inv_sqrt_bc2), F(h.gscale)


def _header(st):
    H = pkg("_hip")
    return H.AmpState.from_buffer_copy(st.raw.cpu().numpy().tobytes())


# ------------------------------------------------------------------------------------------------ a. the Adam bodies, bitwise
@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("n", R.SIZES_ADAM)
def test_adam_is_the_statement_bitwise(n, guarded):
    """k_adam / k_adam_guarded: three steps that carry p, m and v, every (moments, gscale, eps) combination."""
    ops = pkg("ops")
    st = ops.AmpState(torch.device("cuda"), 1.0) if guarded else None
    for ci, (nz, gs, eps) in enumerate(COMBOS):
        c = R.adam_case(n, ci, nz)
        P, M, V, G = Guarded(c["p"]), Guarded(c["m"]), Guarded(c["v"]), Guarded(c["g"][0])
        p, m, v = c["p"], c["m"], c["v"]
        for t in range(1, 4):
            G.set(c["g"][t - 1])
            if guarded:
                lr1, isb, gk = _clean_state(ops, st, gs, t)
                assert gk == F(gs)
                ops.adam_step_guarded(P.view, G.view, M.view, V.view, B1, B2, eps, st)
            else:
                lr1, isb, gk = R.adam_scalars(LR, B1, B2, t) + (gs,)
                ops.adam_step(P.view, G.view, M.view, V.view, LR, B1, B2, eps, t, gs)
            p, m, v, _ = R.adam_ref(p, c["g"][t - 1], m, v, lr1, isb, gk, B1, B2, eps)
            what = "n %d combo %d step %d" % (n, ci, t)
            for got, want, name in ((M, m, "m"), (V, v, "v"), (P, p, "p")):
                _same(got.get(), want, what + " " + name)
            _intact((P, G, M, V), what)
        if guarded:                                                           # found_inf: nothing is stored
            st.found_inf.fill_(1)
            ops.adam_step_guarded(P.view, G.view, M.view, V.view, B1, B2, eps, st)
            for got, want, name in ((M, m, "m"), (V, v, "v"), (P, p, "p")):
                _same(got.get(), want, "n %d combo %d skipped %s" % (n, ci, name))
            _intact((P, G, M, V), "skipped")


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("n", R.SIZES_STRIDE)
def test_adamw_ema_is_the_statement_bitwise(n, shape, guarded):
    """k_adamw_ema_flat / _stride, with and without a state: every mask under every ema_omd and without an average, the (moments,
    gscale, eps) combinations rotated over them; three steps that carry p, m, v and e."""
    ops = pkg("ops")
    st = ops.AmpState(torch.device("cuda"), 1.0) if guarded else None
    ci = 0
    for kind in R.MASK_KINDS:
        words, Wd = _mask(kind, n)
        dec = R.expand_mask(words, n)
        for omd in R.OMDS + (None,):
            nz, gs, eps = COMBOS[ci % len(COMBOS)]
            c = R.adam_case(n, ci, nz)
            ci += 1
            P, M, V, G = Guarded(c["p"]), Guarded(c["m"]), Guarded(c["v"]), Guarded(c["g"][0])
            E = Guarded(c["e"]) if omd is not None else None
            p, m, v, e = c["p"], c["m"], c["v"], c["e"] if omd is not None else None
            for t in range(1, 4):
                G.set(c["g"][t - 1])
                args = (DM, None if Wd is None else Wd.view, None if E is None else E.view, 0.0 if omd is None else omd)
                if guarded:
                    lr1, isb, gk = _clean_state(ops, st, gs, t)
                    ops.adamw_ema_step(P.view, G.view, M.view, V.view, 123.0, B1, B2, eps, 0, 77.0, *args, st)     # lr, step, gscale ignored
                else:
                    lr1, isb, gk = R.adam_scalars(LR, B1, B2, t) + (gs,)
                    ops.adamw_ema_step(P.view, G.view, M.view, V.view, LR, B1, B2, eps, t, gs, *args)
                p, m, v, e = R.adam_ref(p, c["g"][t - 1], m, v, lr1, isb, gk, B1, B2, eps, DM, dec, e, 0.0 if omd is None else omd)
                what = "n %d %s mask %s omd %r step %d" % (n, shape, kind, omd, t)
                for got, want, name in ((M, m, "m"), (V, v, "v"), (P, p, "p"), (E, e, "e")):
                    if got is not None:
                        _same(got.get(), want, what + " " + name)
                _intact((P, G, M, V, E, Wd), what)
            if guarded:                                                       # found_inf: nothing is stored, the average included
                st.found_inf.fill_(1)
                ops.adamw_ema_step(P.view, G.view, M.view, V.view, LR, B1, B2, eps, 0, 1.0, *args, st)
                for got, want, name in ((M, m, "m"), (V, v, "v"), (P, p, "p"), (E, e, "e")):
                    if got is not None:
                        _same(got.get(), want, "n %d %s mask %s skipped %s" % (n, shape, kind, name))
                _intact((P, G, M, V, E, Wd), "skipped")


# ------------------------------------------------------------------------------------------------ b. k_grad_stats
def _parts(st):
    H = pkg("_hip")
    a, b = H.AmpState.part_sum.offset // 4, H.AmpState.part_flag.offset // 4
    return st.raw[a:a + R.AMP_PARTS], st.raw[b:b + R.AMP_PARTS].view(torch.int32)


def _stats(ops, st, view):
    """dcf_grad_stats over poisoned partials: (per-workgroup sums as exact int64, flags), both on the host."""
    ps, pf = _parts(st)
    ps.fill_(-5.0)
    pf.fill_(-5)
    ops.grad_stats(view, st)
    ps, pf = ps.cpu().numpy(), pf.cpu().numpy()
    return ps, pf


def _total(ps):
    """The integer the partials add up to; every partial an integer below 2^24, so every fp32 add that formed it was exact."""
    bad = ~(np.isfinite(ps) & (ps == np.round(ps)) & (ps < 2.0 ** 24) & (ps >= 0.0))
    assert not bad.any(), "partials %s are %s: not integers in [0, 2^24)" % (np.nonzero(bad)[0][:8], ps[bad][:8])
    return int(ps.astype(np.int64).sum())


def _block_of(pos, n):
    """The workgroup that reads element pos: float4 i belongs to lane i % stride; the tail to workgroup 0."""
    return ((pos // 4) % S) // R.THREADS if pos < 4 * (n >> 2) else 0


def _nan_guarded(n):
    """n zeros between NaN canaries: a load past either end raises the flag and poisons the sum."""
    g = Guarded(torch.zeros(n, device="cuda"), float("nan"))
    return g


@pytest.fixture(scope="module")
def small_ints():
    n = 4 * max(R.SIZES_STATS_N4) + 3
    gen = torch.Generator(device="cuda").manual_seed(11)
    return torch.randint(-3, 4, (n,), generator=gen, device="cuda").to(torch.float32)


@pytest.mark.parametrize("n4", R.SIZES_STATS_N4)
def test_grad_stats_counts_every_element_once(n4, small_ints):
    """All ones: the partials add up to n.  Integers in [-3, 3]: to the exact sum of squares.  No flag, and the scale is latched."""
    ops = pkg("ops")
    st = ops.AmpState(torch.device("cuda"), 8.0)
    for tail in R.STATS_TAILS:
        n = 4 * n4 + tail
        G = _nan_guarded(n)
        G.view.fill_(1.0)
        st.scale_in.fill_(-1.0)
        ps, pf = _stats(ops, st, G.view)
        assert _total(ps) == n and not pf.any(), (n, _total(ps))
        assert float(st.scale_in.item()) == 8.0
        G.view.copy_(small_ints[:n])
        want = int((small_ints[:n].to(torch.int64) ** 2).sum().item())
        ps, pf = _stats(ops, st, G.view)
        assert _total(ps) == want and not pf.any(), (n, _total(ps), want)
        assert G.intact()
        if n == 0:                                                            # nothing read: norm 0, coefficient exactly 1
            ops.amp_update(st, 0.5, False, 2.0, 0.5, 2000, 1.0, LR, B1, B2)
            h = _header(st)
            assert (h.grad_norm, h.clip_coef, h.found_inf, h.applied_steps) == (0.0, 1.0, 0, 1)


def _one_hot(ops, st, G, n, positions):
    for pos in positions:
        blk = _block_of(pos, n)
        G.view[pos] = 1.0
        ps, pf = _stats(ops, st, G.view)
        assert _total(ps) == 1 and ps[blk] == 1.0 and not pf.any(), (n, pos, _total(ps), blk)
        for bad in (float("inf"), float("-inf"), float("nan")):
            G.view[pos] = bad
            ps, pf = _stats(ops, st, G.view)
            assert pf[blk] == 1 and int(pf.sum()) == 1, (n, pos, bad, np.nonzero(pf)[0])
            ops.amp_update(st, 1.0, False, 2.0, 0.5, 2000, None, LR, B1, B2)
            assert int(st.found_inf.item()) == 1, (n, pos, bad)
        G.view[pos] = 0.0
    assert G.intact()


@pytest.mark.parametrize("n", [4 * (4 * S + 1) + 3, 4 * (3 * S) + 1])
def test_grad_stats_one_hot_at_every_path(n):
    """Zero but for one element, at every position that names a path of the kernel: a single 1.0 sums to exactly 1 in the
    workgroup that owns it; inf, -inf and NaN there raise that workgroup's flag alone and found_inf."""
    ops = pkg("ops")
    st = ops.AmpState(torch.device("cuda"), 1.0)
    pos = R.stats_positions(n)
    assert len(pos) >= 2 * 8 + (n & 3)
    _one_hot(ops, st, _nan_guarded(n), n, pos)
    assert int(st.applied_steps.item()) == 0 and int(st.skipped_steps.item()) == 3 * len(pos)


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_grad_stats_small_sizes(n, small_ints):
    """Only the tail (and at 5 one float4) runs: all ones, integers, one-hot and the non-finite probes at every element."""
    ops = pkg("ops")
    st = ops.AmpState(torch.device("cuda"), 1.0)
    G = _nan_guarded(n)
    G.view.fill_(1.0)
    ps, pf = _stats(ops, st, G.view)
    assert _total(ps) == n and not pf.any()
    G.view.copy_(small_ints[100:100 + n])
    ps, pf = _stats(ops, st, G.view)
    assert _total(ps) == int((small_ints[100:100 + n].to(torch.int64) ** 2).sum().item()) and not pf.any()
    G.view.fill_(0.0)
    _one_hot(ops, st, G, n, range(n))


@pytest.mark.parametrize("n", [3, 4099])
def test_grad_stats_raises_no_false_flag(n):
    """FLT_MAX, denormals and -0.0 are finite: no flag, and without clipping the step is applied although the sum of squares
    overflows (grad_norm is inf).  With clipping on the infinite norm itself skips the step, as the header states."""
    ops = pkg("ops")
    fmax = float(np.finfo(F).max)
    x = np.random.RandomState(n).uniform(-1, 1, n).astype(F)
    for k, val in enumerate((fmax, -fmax, 1e-40, -1e-45, -0.0)):
        x[(k * 1021) % n if n > 8 else k % n] = F(val)
    x[n - 1] = F(-fmax)                                                       # the ragged tail
    G = Guarded(x, float("nan"))
    st = ops.AmpState(torch.device("cuda"), 1.0)
    ps, pf = _stats(ops, st, G.view)
    assert not pf.any() and np.isinf(ps).any() and not np.isnan(ps).any()
    ops.amp_update(st, 1.0, False, 2.0, 0.5, 2000, None, LR, B1, B2)
    h = _header(st)
    assert (h.found_inf, h.applied_steps, h.skipped_steps, h.grad_norm, h.clip_coef, h.gscale) == (0, 1, 0, float("inf"), 1.0, 1.0)
    ps, pf = _stats(ops, st, G.view)
    ops.amp_update(st, 1.0, False, 2.0, 0.5, 2000, 1.0, LR, B1, B2)
    h = _header(st)
    assert (h.found_inf, h.applied_steps, h.skipped_steps, h.grad_norm, h.clip_coef) == (1, 1, 1, float("inf"), 1.0)
    assert not pf.any() and G.intact()


def test_grad_norm_against_the_statement():
    """grad_norm = float32(sqrt(float64(sum)) * |gscale_host| / S).  Bitwise where the sum is a perfect square (all ones at n = 4, 9,
    1024, 4 194 304: the square root is exact and the product and quotient are IEEE double operations); elsewhere at most 1 fp32
    ulp -- the device's double sqrt is not promised correctly rounded, and a few double ulps move a float rounding by one step at
    most.  The number of non-bitwise cases is printed."""
    ops = pkg("ops")
    st = ops.AmpState(torch.device("cuda"), 3.0)
    squares = (4, 9, 1024, 4194304)
    loose = 0
    ones = torch.ones(max(squares) + 16, device="cuda")
    for n in squares + (1, 2, 3, 5, 7, 1023, 1025, 4099, 4 * S + 7):
        G = Guarded(ones[:n], float("nan"))
        ps, pf = _stats(ops, st, G.view)
        ops.amp_update(st, 0.37, False, 2.0, 0.5, 2000, None, LR, B1, B2)
        total = R.sum_partials(ps)
        assert total == float(n)
        want = R.amp_update_ref(dict({k: 0 for k in R.STATE_FIELDS}, scale_in=3.0), total, 0, 0.37, False, 2.0, 0.5, 2000, None, LR, B1, B2)
        got = F(st.grad_norm.item())
        d = R.ulps_apart(got, want["grad_norm"])
        assert d <= (0 if n in squares else 1), (n, got, want["grad_norm"])
        loose += d != 0
    print("grad_norm: %d of %d cases not bitwise (1 ulp)" % (loose, len(squares) + 9))


# ------------------------------------------------------------------------------------------------ c. k_amp_update
FMAX = float(np.finfo(F).max)


def _case(name, grad=(3.0, 4.0), scale=8.0, tracker=0, applied=0, skipped=0, gscale_host=0.5, dynamic=False, growth=2.0, backoff=0.5,
          interval=2000, max_norm=None, latch=None):
    return dict(name=name, grad=grad, scale=scale, tracker=tracker, applied=applied, skipped=skipped, gscale_host=gscale_host,
                dynamic=dynamic, growth=growth, backoff=backoff, interval=interval, max_norm=max_norm, latch=latch)


AMP_CASES = [
    _case("static clean"),
    _case("static found", grad=(3.0, float("inf")), tracker=5),
    _case("dynamic clean, tracker below the interval", dynamic=True, interval=3),
    _case("dynamic clean, tracker reaches interval 3", dynamic=True, interval=3, tracker=2),
    _case("dynamic clean, interval 1", dynamic=True, interval=1),
    _case("dynamic found", grad=(float("nan"), 4.0), dynamic=True, interval=3, tracker=2),
    _case("growth from 2^127 would be inf", dynamic=True, interval=1, scale=2.0 ** 127),
    _case("backoff 0.75", grad=(float("-inf"), 0.0), dynamic=True, scale=1000.0, backoff=0.75),
    _case("scale 750, clipped: the order of gscale_host / S * coef", scale=750.0, gscale_host=0.37, max_norm=0.001),
    _case("max_norm above the norm: coefficient exactly 1", max_norm=10.0),
    _case("max_norm below the norm", max_norm=0.1),
    _case("norm zero while clipping", grad=(0.0, -0.0), max_norm=1.0),
    _case("infinite norm while clipping: skipped", grad=(FMAX, 1.0), max_norm=1.0, dynamic=True, tracker=1),
    _case("infinite norm without clipping: applied", grad=(FMAX, 1.0)),
    _case("scale_in latch", scale=8.0, latch=16.0, max_norm=0.1),
    _case("scale_in latch, dynamic growth", scale=8.0, latch=64.0, dynamic=True, interval=1),
    _case("skipped_steps over 2^31", grad=(float("inf"), 1.0), skipped=2 ** 31 + 5, applied=2 ** 31 + 5),
] + [_case("applied_steps %d" % a, applied=a, max_norm=0.1) for a in (0, 1, 9, 999, 10 ** 5, 10 ** 7, 2 ** 31 + 5)]
PREFILL = {"grad_norm": -80.25, "clip_coef": -81.25, "gscale": -77.25, "lr_over_bc1": -78.25, "inv_sqrt_bc2": -79.25}


def test_amp_update_table():
    """Every field of the state's header after dcf_grad_stats + dcf_amp_update against amp_update_ref, from fields the test wrote
    itself; the Adam scalars are pre-filled with canaries, so "not written on a skipped step" shows.  Bitwise, except lr_over_bc1
    and inv_sqrt_bc2 while b^t >= 2^-54: the device's double pow is not promised correctly rounded, which may move the float
    rounding by one step (1 ulp allowed, the count printed)."""
    ops = pkg("ops")
    loose = compared = 0
    for c in AMP_CASES:
        st = ops.AmpState(torch.device("cuda"), c["scale"])
        st.scale_in.fill_(-3.0)                                               # dcf_grad_stats latches it from scale_next
        st.growth_tracker.fill_(c["tracker"])
        st.found_inf.fill_(7)
        st.applied_steps.fill_(c["applied"])
        st.skipped_steps.fill_(c["skipped"])
        for k, val in PREFILL.items():
            getattr(st, k).fill_(val)
        g = np.array(c["grad"], dtype=F)
        G = Guarded(g, float("nan"))
        ops.grad_stats(G.view, st)
        if c["latch"] is not None:
            st.scale_next.fill_(c["latch"])
        ops.amp_update(st, c["gscale_host"], c["dynamic"], c["growth"], c["backoff"], c["interval"], c["max_norm"], LR, B1, B2)
        got = _header(st)
        with np.errstate(all="ignore"):
            sq = g * g
            sum_sq = float(np.float64(sq[0]) + np.float64(sq[1]))
        before = dict(PREFILL, scale_in=c["scale"], scale_next=c["scale"] if c["latch"] is None else c["latch"], growth_tracker=c["tracker"],
                      found_inf=7, applied_steps=c["applied"], skipped_steps=c["skipped"])
        want = R.amp_update_ref(before, sum_sq, not np.isfinite(g).all(), c["gscale_host"], c["dynamic"], c["growth"], c["backoff"],
                                c["interval"], c["max_norm"], LR, B1, B2)
        t = want["applied_steps"]
        for k in R.STATE_FIELDS:
            a, b = getattr(got, k), want[k]
            if k not in R.STATE_FLOATS:
                assert a == int(b), (c["name"], k, a, b)
            elif k in ("lr_over_bc1", "inv_sqrt_bc2") and not want["found_inf"] and not R.bias_is_exactly_one(B1 if k == "lr_over_bc1" else B2, t):
                d = R.ulps_apart(a, b)
                assert d <= 1, (c["name"], k, a, b)
                loose, compared = loose + (d != 0), compared + 1
            else:
                assert R.same_bits(F(a), F(b)).all(), (c["name"], k, a, float(b))
        assert G.intact()
    print("amp_update: %d of %d Adam scalars with b^t >= 2^-54 not bitwise (1 ulp)" % (loose, compared))
    # what the table is meant to reach
    names = {c["name"]: c for c in AMP_CASES}
    assert len(names) == len(AMP_CASES) and compared >= 10


# ------------------------------------------------------------------------------------------------ d. FlatAdam.step on a stub model
class _Table(object):
    # (key, logical shape, offset, physical numel, layout): two weights and an excluded bias, each starting a float4 group
    entries = [("l1.weight", (5, 7), 0, 35, "plain"), ("l1.bias", (6,), 36, 6, "plain"), ("l2.weight", (5, 7), 44, 35, "plain")]


N_STUB = 79


class _Stub(object):
    def __init__(self, p):
        self.P, self.G = Guarded(p), Guarded(np.zeros(N_STUB, dtype=F))
        self.flat_params, self.flat_grads, self._table = self.P.view, self.G.view, _Table()


SCHEDULE = {"kind": "cosine", "warmup_steps": 2, "warmup_start_factor": 0.1, "total_steps": 10, "min_lr": 1e-5}


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("recipe", ["adam", "adamw_ema"])
def test_flat_adam_step_branches(recipe, guarded):
    """FlatAdam.step: three calls with a fresh gradient each and gscale 0.5; after each, p, m, v and the average equal adam_ref fed
    optim.lr_at, float32(1 - lr * wd), 1 - optim.ema_decay_at and optim.decay_bits (and, when guarded, the scalars read from the
    state, themselves checked against the scheduled rate).  The guarded runs' second call holds an inf: it leaves the four arrays and
    applied_steps as they were, while opt_calls advances."""
    TR, OPT = pkg("train"), pkg("optim")
    cfg = {"lr_schedule": SCHEDULE}
    if recipe == "adamw_ema":
        cfg.update(weight_decay=0.01, ema_decay=0.99)
    rec = OPT.parse_optim_config(cfg)
    guard = TR.parse_guard_config({"loss_scale": "dynamic", "loss_scale_init": 4.0, "loss_scale_growth_interval": 2}) if guarded else None
    rng = np.random.RandomState(21)
    p = rng.uniform(-1, 1, N_STUB).astype(F)
    model = _Stub(p)
    opt = TR.FlatAdam(model, 2e-3, (B1, B2), guard=guard, recipe=rec)
    fused = recipe == "adamw_ema"
    assert opt.fused == fused and (opt.ema is not None) == fused and (opt.decay_bits is not None) == fused
    dec = R.expand_mask(OPT.decay_bits(_Table.entries, N_STUB, rec["weight_decay_exclude"]), N_STUB) if fused else None
    if fused:
        assert dec[:36].all() and not dec[36:44].any() and dec[44:].all()
    m, v, e = np.zeros(N_STUB, dtype=F), np.zeros(N_STUB, dtype=F), p.copy() if fused else None
    applied = 0
    for k in range(3):
        g = rng.uniform(-1, 1, N_STUB).astype(F)
        skip = guarded and k == 1
        if skip:
            g[37] = np.inf
        model.G.set(g)
        opt.step(0.5)
        lr = OPT.lr_at(rec["schedule"], 2e-3, k)
        assert opt.opt_calls == k + 1
        if guarded:
            h = _header(opt.amp)
            assert h.found_inf == int(skip) and h.applied_steps == applied + (not skip) and h.skipped_steps == (k >= 1)
        if not skip:
            applied += 1
            if guarded:
                lr1, isb, gk = F(h.lr_over_bc1), F(h.inv_sqrt_bc2), F(h.gscale)
                w1, w2 = R.adam_scalars(lr, B1, B2, applied)
                assert R.ulps_apart(lr1, w1) <= 1 and R.ulps_apart(isb, w2) <= 1 and gk == F(0.5) / F(h.scale_in), (k, lr1, w1, isb, w2, gk)
            else:
                lr1, isb, gk = R.adam_scalars(lr, B1, B2, applied) + (0.5,)
            decay_mul = F(1.0 - lr * rec["weight_decay"]) if fused else 1.0
            omd = F(1.0 - OPT.ema_decay_at(rec, k)) if fused else 0.0
            p, m, v, e = R.adam_ref(p, g, m, v, lr1, isb, gk, B1, B2, 1e-8, decay_mul, dec, e, omd)
        what = "%s %s call %d" % (recipe, "guarded" if guarded else "plain", k)
        _same(model.P.get(), p, what + " p")
        _same(opt.m.cpu().numpy(), m, what + " m")
        _same(opt.v.cpu().numpy(), v, what + " v")
        if fused:
            _same(opt.ema.cpu().numpy(), e, what + " ema")
        assert model.P.intact() and model.G.intact()
    assert opt.step_count == applied == (2 if guarded else 3)
