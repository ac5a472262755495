"""GPU suite: dcf_adamw_ema_step (csrc/optim.hip) through the C ABI -- bitwise against dcf_adam_step / dcf_adam_step_guarded with the
features off, decoupled decay under a random one-bit-per-float4 mask, the weight average against three eager torch ops, the
guarded form (skip, and equality with the plain call), and torch.optim.AdamW.  Sizes: 4 (one group), 4099 (a ragged tail whose
bit is the only one of the last mask word) and 3080 (block and mask-word boundaries are crossed); both launch shapes."""
import numpy as np
import pytest
import torch

from _util import pkg, rand32, rnd

pytestmark = pytest.mark.gpu

SIZES = [4, 4099, 3080]
SHAPES = ["flat", "stride"]
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
DECAY_MUL = float(np.float32(1.0 - LR * 0.01))


@pytest.fixture(params=SHAPES)
def shape(request):
    H = pkg("_hip")
    H.set_option("ADAMW_SHAPE", request.param)
    yield request.param
    H.set_option("ADAMW_SHAPE", None)


def _mask(n, seed):
    """(uint64 words as an int64 device tensor, per-element bool device tensor) of a random mask from the sampler hash."""
    groups = (n + 3) // 4
    bits = [rand32(seed, 0, 0, j, 0) & 1 for j in range(groups)]
    words = np.zeros((groups + 63) // 64, dtype=np.uint64)
    for j, b in enumerate(bits):
        if b:
            words[j // 64] |= np.uint64(1) << np.uint64(j % 64)
    elem = torch.tensor(bits, dtype=torch.bool).repeat_interleave(4)[:n]
    return torch.from_numpy(words.view(np.int64)).cuda(), elem.cuda()


def _start(n):
    return rnd((n,), 14).cuda(), rnd((n,), 15).cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")


def _adam_ref(ops, p, g, m, v, step, gscale=1.0):
    """dcf_adam_step on copies."""
    p, m, v = p.clone(), m.clone(), v.clone()
    ops.adam_step(p, g, m, v, LR, B1, B2, EPS, step, gscale)
    return p, m, v


@pytest.mark.parametrize("n", SIZES)
def test_features_off_is_the_adam_step(n, shape):
    ops = pkg("ops")
    p, g, m, v = _start(n)
    for step in range(1, 4):
        gg = g * step
        pr, mr, vr = _adam_ref(ops, p, gg, m, v, step, 0.5)
        ops.adamw_ema_step(p, gg, m, v, LR, B1, B2, EPS, step, 0.5)
        assert torch.equal(p, pr) and torch.equal(m, mr) and torch.equal(v, vr), step


@pytest.mark.parametrize("n", SIZES)
def test_decay_under_a_random_mask(n, shape):
    ops = pkg("ops")
    words, elem = _mask(n, 77 + n)
    assert n == 4 or (bool(elem.any()) and not bool(elem.all()))
    p, g, m, v = _start(n)
    pa, ma, va = p.clone(), m.clone(), v.clone()                        # NULL mask against the all-ones mask
    ones = torch.full((((n + 3) // 4 + 63) // 64,), -1, dtype=torch.int64, device="cuda")
    pn, mn, vn = p.clone(), m.clone(), v.clone()
    for step in range(1, 4):
        gg = g * step
        clear = _adam_ref(ops, p, gg, m, v, step)                        # groups with a clear bit
        decayed = _adam_ref(ops, p * DECAY_MUL, gg, m, v, step)         # groups with a set bit: one fp32 multiply in front
        ops.adamw_ema_step(p, gg, m, v, LR, B1, B2, EPS, step, 1.0, DECAY_MUL, words)
        assert torch.equal(p, torch.where(elem, decayed[0], clear[0])), step
        assert torch.equal(m, clear[1]) and torch.equal(v, clear[2]) and torch.equal(m, decayed[1]) and torch.equal(v, decayed[2])
        ops.adamw_ema_step(pa, gg, ma, va, LR, B1, B2, EPS, step, 1.0, DECAY_MUL, ones)
        ops.adamw_ema_step(pn, gg, mn, vn, LR, B1, B2, EPS, step, 1.0, DECAY_MUL, None)
        assert torch.equal(pa, pn) and torch.equal(ma, mn) and torch.equal(va, vn), step
    assert not torch.equal(pa, p) or n == 4


@pytest.mark.parametrize("n", SIZES)
def test_ema_is_three_fp32_ops(n, shape):
    """e' = e + omd * (p' - e), each operation rounded to fp32: a subtraction, a multiplication and an addition as separate eager
    torch kernels (no alpha=, no lerp: those may fuse).  omd = 0 leaves e as it is."""
    ops = pkg("ops")
    words, _ = _mask(n, 5 + n)
    p, g, m, v = _start(n)
    e = rnd((n,), 16).cuda()
    e0 = e.clone()
    still = e.clone()
    ps, ms, vs = p.clone(), m.clone(), v.clone()
    for step, omd in ((1, 0.25), (2, float(np.float32(1e-3))), (3, float(np.float32(0.9)))):
        gg = g * step
        pr, mr, vr = p.clone(), m.clone(), v.clone()
        ops.adamw_ema_step(pr, gg, mr, vr, LR, B1, B2, EPS, step, 1.0, DECAY_MUL, words)      # the same step without the average
        d = pr - e
        d = d * torch.tensor(omd, dtype=torch.float32, device="cuda")
        er = e + d
        ops.adamw_ema_step(p, gg, m, v, LR, B1, B2, EPS, step, 1.0, DECAY_MUL, words, e, omd)
        assert torch.equal(p, pr) and torch.equal(m, mr) and torch.equal(v, vr), step
        assert torch.equal(e, er), step
        ops.adamw_ema_step(ps, gg, ms, vs, LR, B1, B2, EPS, step, 1.0, DECAY_MUL, words, still, 0.0)
        assert torch.equal(still, e0) and torch.equal(ps, p), step
    assert not torch.equal(e, e0)


@pytest.mark.parametrize("n", SIZES)
def test_ema_with_omd_one_follows_the_parameters(n, shape):
    """omd = 1 gives e' = e + (p' - e) = p' wherever the subtraction is exact, i.e. (Sterbenz) where e / 2 <= p' <= 2 e.  The
    average starts as a copy of the parameters, as in the trainer, and the parameters are drawn from +-[0.5, 1): by Cauchy-Schwarz
    |m^| <= sqrt(sum_i w1_i^2 / w2_i) * sqrt(bc2) / bc1 * sqrt(v^) with the moments' weights w1, w2, which is 1.00 at steps 1 to 3,
    so an update is at most lr = 1e-3 (and the decay 1e-5 of p) in magnitude: every p' is within a factor two of its e = p and
    the statement holds for every element.  (On parameters near zero p' - e rounds and e' can miss p'
    by an ulp: the count is printed for the uniform [-1, 1) data of the other tests, without an assertion.)"""
    ops = pkg("ops")
    _, g, m, v = _start(n)
    mag, sign = rnd((n,), 17, 0.5, 1.0), rnd((n,), 18)
    p = torch.where(sign < 0, -mag, mag).cuda()
    e = p.clone()
    q, mq, vq = rnd((n,), 14).cuda(), m.clone(), v.clone()
    eq = q.clone()
    for step in range(1, 4):
        gg = g * step
        ops.adamw_ema_step(p, gg, m, v, LR, B1, B2, EPS, step, 1.0, DECAY_MUL, None, e, 1.0)
        assert torch.equal(e, p), step
        ops.adamw_ema_step(q, gg, mq, vq, LR, B1, B2, EPS, step, 1.0, DECAY_MUL, None, eq, 1.0)
        print("uniform [-1, 1) parameters, step %d: %d of %d elements of e' differ from p'" % (step, int((eq != q).sum()), n))


@pytest.mark.parametrize("n", SIZES)
def test_guarded_skip_and_equality_with_the_plain_call(n, shape):
    ops = pkg("ops")
    words, _ = _mask(n, 9 + n)
    p, g, m, v = _start(n)
    e = rnd((n,), 16).cuda()
    pp, mp, vp, ep = p.clone(), m.clone(), v.clone(), e.clone()
    st = ops.AmpState(torch.device("cuda"), 1.0)
    for step in range(1, 4):
        gg = g * step
        # a clean state from the real pipeline: scale 1, no clipping -> gscale 0.5, and dcf_adam_step's scalars for applied step `step`
        ops.grad_stats(gg, st)
        ops.amp_update(st, 0.5, False, 2.0, 0.5, 2000, None, LR, B1, B2)
        assert int(st.found_inf.item()) == 0 and int(st.applied_steps.item()) == step and float(st.gscale.item()) == 0.5
        ops.adamw_ema_step(p, gg, m, v, 123.0, B1, B2, EPS, 0, 77.0, DECAY_MUL, words, e, 0.125, st)     # lr, step, gscale ignored
        ops.adamw_ema_step(pp, gg, mp, vp, LR, B1, B2, EPS, step, 0.5, DECAY_MUL, words, ep, 0.125)
        assert torch.equal(p, pp) and torch.equal(m, mp) and torch.equal(v, vp) and torch.equal(e, ep), step
    # features off with a state: dcf_adam_step_guarded's stores
    pg, mg, vg = p.clone(), m.clone(), v.clone()
    ops.adam_step_guarded(pg, g, mg, vg, B1, B2, EPS, st)
    ops.adamw_ema_step(p, g, m, v, LR, B1, B2, EPS, 0, 1.0, 1.0, None, None, 0.0, st)
    assert torch.equal(p, pg) and torch.equal(m, mg) and torch.equal(v, vg)
    # found_inf: nothing is stored, the average included
    st.found_inf.fill_(1)
    before = [t.clone() for t in (p, m, v, e)]
    ops.adamw_ema_step(p, g, m, v, LR, B1, B2, EPS, 0, 1.0, DECAY_MUL, words, e, 0.5, st)
    ops.adamw_ema_step(p, g, m, v, LR, B1, B2, EPS, 0, 1.0, DECAY_MUL, None, None, 0.0, st)
    assert all(torch.equal(a, b) for a, b in zip((p, m, v, e), before))


@pytest.mark.parametrize("n", SIZES)
def test_adamw_matches_torch(n, shape):
    """torch.optim.AdamW, weight_decay 0.01 on every element, three steps: the bound of test_adam_matches_torch."""
    ops = pkg("ops")
    p0, g = rnd((n,), 14), rnd((n,), 15)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=0.01)
    pd, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for step in range(1, 4):
        gg = g * step
        p.grad = gg.clone()
        opt.step()
        ops.adamw_ema_step(pd, gg.cuda(), m, v, LR, B1, B2, EPS, step, 1.0, 1.0 - LR * 0.01)
        assert torch.allclose(pd.cpu(), p.detach(), rtol=1e-6, atol=1e-7), step


def test_grid_stride_trips_equal_the_flat_shape():
    """The capped grid walks more than one chunk per workgroup only above 2048 * 512 groups: at 2 * 2048 * 512 groups + a ragged
    tail (8.4 M elements) the stride shape's stores equal the flat shape's, decay mask, average and guard state included."""
    H, ops = pkg("_hip"), pkg("ops")
    n = 2 * 2048 * 512 * 4 + 4099
    gen = torch.Generator().manual_seed(3)
    p0, g, e0 = (torch.rand(n, generator=gen) * 2 - 1).cuda(), (torch.rand(n, generator=gen) * 2 - 1).cuda(), (torch.rand(n, generator=gen) * 2 - 1).cuda()
    words = torch.randint(-2 ** 63, 2 ** 63 - 1, (((n + 3) // 4 + 63) // 64,), generator=gen, dtype=torch.int64).cuda()
    st = ops.AmpState(torch.device("cuda"), 1.0)
    ops.grad_stats(g, st)
    ops.amp_update(st, 1.0, False, 2.0, 0.5, 2000, None, LR, B1, B2)
    out = {}
    try:
        for shape in SHAPES:
            H.set_option("ADAMW_SHAPE", shape)
            p, m, v, e = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), e0.clone()
            ops.adamw_ema_step(p, g, m, v, LR, B1, B2, EPS, 1, 1.0, DECAY_MUL, words, e, 0.25)
            ops.adamw_ema_step(p, g, m, v, LR, B1, B2, EPS, 0, 1.0, DECAY_MUL, None, e, 0.25, st)
            out[shape] = (p, m, v, e)
    finally:
        H.set_option("ADAMW_SHAPE", None)
    assert all(torch.equal(a, b) for a, b in zip(out["flat"], out["stride"]))
    assert not torch.equal(out["flat"][0], p0) and not torch.equal(out["flat"][3], e0)
