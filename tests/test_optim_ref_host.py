"""The fp32 statements of tests/_optim_ref.py against fp64 torch.optim.Adam / AdamW, torch._amp_update_scale_ and clip_grad_norm_,
the mask expansion against a hand-written bit list, and stats_positions against a literal walk of k_grad_stats' loops -- so that a
wrong statement cannot bless a wrong kernel (tests/test_gpu_optim_edges.py).  CPU only."""
import math

import numpy as np
import pytest
import torch

import _amp_ref as A
import _optim_ref as R

F = np.float32
U = 2.0 ** -24                          # half an ulp, relative: one fp32 rounding


# ---------------------------------------------------------------------------------------------------------------- adam_ref
def _torch_steps(kind, p0, grads, m0, v0, lr, b1, b2, eps, wd):
    """fp64 torch.optim.Adam / AdamW from the given moments; the (p, m, v) after each step."""
    p = torch.tensor(p0, dtype=torch.float64).requires_grad_(True)
    cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    opt = cls([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd if kind == "adamw" else 0.0, foreach=False)
    opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.tensor(m0, dtype=torch.float64),
                    "exp_avg_sq": torch.tensor(v0, dtype=torch.float64)}
    out = []
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
    return out


@pytest.mark.parametrize("kind", ["adam", "adamw"])
@pytest.mark.parametrize("nonzero", [False, True])
@pytest.mark.parametrize("gscale", [1.0, 0.37])
def test_adam_ref_against_fp64_torch(kind, nonzero, gscale):
    """Three steps on ordinary data (no edge values).  torch gets the fp32 inputs and the fp32-rounded lr, betas and eps as exact
    doubles (and the gradient times gscale in fp64), so every difference is a rounding of the statement.  The bound counts them, to
    first order in U = 2^-24 (one fp32 rounding = half an ulp), carried from step to step per element:
        gk                    1 rounding (the product with gscale)
        m' = b1*m + c1*gk     5: b1*m; gk, c1 = fl(1-b1) and their product (3 on the second term); the sum
              em' <= b1*em + U*(|b1*m| + 3*|c1*gk| + |m'|)
        v' = b2*v + c2*gk*gk  7: b2*v; c2 = fl(1-b2), gk twice, two products (5 on the second term); the sum
              ev' <= b2*ev + U*(|b2*v| + 5*|c2*gk*gk| + |v'|)
        r = num / den         7: lr_over_bc1, its product with m' (2 on num); sqrt, inv_sqrt_bc2, their product, the sum with eps
                              (4 on den, each at most U*den); the quotient
              er <= (lr1*em' + 2*U*|num|)/den + |r|*(isb*ev'/(2*sqrt(v')) + 4*U*den)/den + U*|r|
        p' = q - r            2 (3 with decay: decay_mul = fl(1 - lr*wd) and the product): ep' <= ep + [2*U*|q|] + er + U*|p'|
    21 or 22 roundings a step.  Where nothing cancels this is U * |p'| + about 19 * U * |r| per step (3 * U * |p| + 57 * U * |r| =
    3 * 2^-24 for |p| near 1 and lr-sized updates over the three steps); the per-element form also covers a first moment that
    cancels and the large updates of a small second moment.  The factor 1.001 covers the second-order terms
    ((1 + U)^22 - 1 < 22 * U * 1.001).  The largest bound is printed as a multiple of 2^-24."""
    n, wd = 4099, 0.01
    c = R.adam_case(n, 3 + int(nonzero), nonzero, edges=False)
    lr, b1, b2, eps = (float(F(x)) for x in (R.LR, R.B1, R.B2, R.EPS))
    decay_mul = 1.0 - lr * wd if kind == "adamw" else 1.0
    want = _torch_steps(kind, c["p"], [g.astype(np.float64) * float(F(gscale)) for g in c["g"]], c["m"], c["v"], lr, b1, b2, eps, wd)
    p, m, v = c["p"], c["m"], c["v"]
    ep, em, ev = np.zeros(n), np.zeros(n), np.zeros(n)
    P, M, V = (x.astype(np.float64) for x in (p, m, v))                 # torch's values before the step
    worst = 0.0
    for t in range(1, 4):
        lr1, isb = R.adam_scalars(lr, b1, b2, t)
        p, m, v, _ = R.adam_ref(p, c["g"][t - 1], m, v, lr1, isb, gscale, b1, b2, eps, decay_mul)
        Pn, Mn, Vn = want[t - 1]
        gk = c["g"][t - 1].astype(np.float64) * float(F(gscale))
        em = b1 * em + U * (np.abs(b1 * M) + 3 * np.abs((1 - b1) * gk) + np.abs(Mn))
        ev = b2 * ev + U * (np.abs(b2 * V) + 5 * np.abs((1 - b2) * gk * gk) + np.abs(Vn))
        sq = np.sqrt(Vn)
        assert float(sq.min()) > 0.0                                     # ordinary data: no zero second moment
        den = sq * float(isb) + eps
        num = float(lr1) * Mn
        r = num / den
        er = (float(lr1) * em + 2 * U * np.abs(num)) / den + np.abs(r) * (float(isb) * ev / (2 * sq) + 4 * U * den) / den + U * np.abs(r)
        q = P * decay_mul
        ep = ep + (2 * U * np.abs(q) if kind == "adamw" else 0.0) + er + U * np.abs(Pn)
        for got, ref, err, what in ((p, Pn, ep, "p"), (m, Mn, em, "m"), (v, Vn, ev, "v")):
            d = np.abs(got.astype(np.float64) - ref)
            assert np.all(d <= 1.001 * err), "%s step %d: off by %g, bound %g" % (what, t, float(d.max()), float((1.001 * err)[d.argmax()]))
        worst = max(worst, float(np.abs(p.astype(np.float64) - Pn).max()))
        P, M, V = Pn, Mn, Vn
    print("%s nonzero=%s gscale=%g: max |p - p64| %.3g, largest bound %.3g = %.1f * 2^-24" % (kind, nonzero, gscale, worst,
                                                                                              float(ep.max()), float(ep.max()) / U))


@pytest.mark.parametrize("eps", [1e-8, 0.0])
@pytest.mark.parametrize("gscale", [1.0, 0.37])
def test_finite_value_inventory_of_the_edge_vector(eps, gscale):
    """Step 1 from zero moments over the 36 edge pairs: which results are finite, +-inf or NaN, by reasoning, for every g edge (the
    p edge does not change the class: 1e30 stays finite, and -inf swallows it):
        +-0     m' = v' = 0.  eps > 0: update 0 / eps = 0, p' = q.  eps = 0: 0 / 0 = NaN
        1e-40   gk and m' denormal, v' = (c2*gk)*gk underflows to 0.  eps > 0: a tiny finite update.  eps = 0: num / 0 = +inf, p' = -inf
        1e-20   v' denormal but not zero: finite
        1e20    v' about 1e37: finite
        +-3e38  (c2*gk)*gk overflows: v' = +inf, den = +inf, update +-0: p' = q finite, m' finite
        inf     m' = v' = +inf: inf / inf = NaN in p'
        nan     NaN everywhere"""
    n = R.N_EDGES
    c = R.adam_case(n, 1, False)
    lr1, isb = R.adam_scalars(R.LR, R.B1, R.B2, 1)
    p, m, v, _ = R.adam_ref(c["p"], c["g"][0], c["m"], c["v"], lr1, isb, gscale, R.B1, R.B2, eps, R.DECAY_MUL)
    zero = "nan" if eps == 0.0 else "fin"
    want = {"+0": (zero, "fin", "fin"), "-0": (zero, "fin", "fin"), "1e-40": ("-inf" if eps == 0.0 else "fin", "fin", "fin"),
            "1e-20": ("fin", "fin", "fin"), "1e20": ("fin", "fin", "fin"), "3e38": ("fin", "fin", "+inf"), "-3e38": ("fin", "fin", "+inf"),
            "inf": ("nan", "+inf", "+inf"), "nan": ("nan", "nan", "nan")}

    def cls(x):
        return "nan" if np.isnan(x) else "+inf" if x == np.inf else "-inf" if x == -np.inf else "fin"

    names = R.edge_values()["g_names"]
    slots = R.edge_slots(n)
    assert sorted((gi, pi) for _, gi, pi in slots) == [(a, b) for a in range(9) for b in range(4)]
    for i, gi, pi in slots:
        assert (cls(p[i]), cls(m[i]), cls(v[i])) == want[names[gi]], (names[gi], pi, p[i], m[i], v[i])
    # the denormal edges stay denormal (nothing flushed), and v' of 1e-40 is a true zero
    i40 = [i for i, gi, _ in slots if names[gi] == "1e-40"]
    i20 = [i for i, gi, _ in slots if names[gi] == "1e-20"]
    tiny = float(np.finfo(F).tiny)
    assert all(0.0 < m[i] < tiny and v[i] == 0.0 for i in i40) and all(0.0 < v[i] < tiny for i in i20)


# ---------------------------------------------------------------------------------------------------------------- amp_update_ref
def _state(scale, tracker=0, applied=0, skipped=0):
    return {"scale_in": F(scale), "scale_next": F(scale), "growth_tracker": tracker, "found_inf": 0, "applied_steps": applied,
            "skipped_steps": skipped, "grad_norm": F(0), "clip_coef": F(0), "gscale": F(-7), "lr_over_bc1": F(-8), "inv_sqrt_bc2": F(-9)}


SEQUENCES = {
    "backoff": ([1, 1, 0, 1], 65536.0, 2.0, 0.5, 3),
    "growth_interval_3": ([0, 0, 0, 0, 0, 0, 1, 0, 0, 0], 4.0, 2.0, 0.5, 3),
    "growth_interval_1": ([0, 0, 1, 0, 0], 4.0, 2.0, 0.5, 1),
    "growth_overflows": ([0, 0, 0, 1, 0, 0], 2.0 ** 126, 2.0, 0.5, 1),
    "odd_factors": ([0, 1, 0, 0, 1, 1, 0, 0, 0], 1000.0, 1.7, 0.75, 2),
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_amp_update_ref_scale_rule_against_torch(name):
    found, init, growth, backoff, interval = SEQUENCES[name]
    want = A.torch_schedule(found, init, growth, backoff, interval)
    assert want == A.scale_schedule(found, init, growth, backoff, interval)
    st = _state(init)
    applied = skipped = 0
    for bad, (scale, tracker) in zip(found, want):
        st["scale_in"] = st["scale_next"]                                # dcf_grad_stats' latch
        st = R.amp_update_ref(st, math.inf if bad else 25.0, bad, 1.0, True, growth, backoff, interval, None, R.LR, R.B1, R.B2)
        applied, skipped = applied + (not bad), skipped + bool(bad)
        assert (float(st["scale_next"]), st["growth_tracker"]) == (scale, tracker)
        assert (st["found_inf"], st["applied_steps"], st["skipped_steps"]) == (int(bad), applied, skipped)
    if name == "growth_overflows":
        assert float(st["scale_next"]) == 2.0 ** 127 and want[:3] == [(2.0 ** 127, 0)] * 3        # 2^128 is inf: the scale stays
    # the static scale never moves, whatever is found
    st = _state(init, tracker=2)
    for bad in found:
        st = R.amp_update_ref(st, 25.0, bad, 1.0, False, growth, backoff, interval, None, R.LR, R.B1, R.B2)
        assert float(st["scale_next"]) == float(F(init)) and st["growth_tracker"] == 2


@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1000.0])
def test_amp_update_ref_clip_coefficient_against_clip_grad_norm(max_norm):
    """norm, norm + 1e-6f and the quotient round once each, 1e-6f itself is rounded: 4 roundings, 4 * 2^-24 relative on the
    coefficient; exactly 1.0 where torch's is clamped."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(37, generator=g, dtype=torch.float64).requires_grad_(True)
    S, gs = 8.0, 0.5
    x.grad = x.detach().clone()
    total = float(torch.nn.utils.clip_grad_norm_([x], max_norm))
    coef = min(1.0, max_norm / (total + 1e-6))
    arena = x.detach().numpy() * S / gs                                   # what the scaled, unaveraged arena holds
    st = R.amp_update_ref(_state(S), float((arena ** 2).sum()), 0, gs, False, 2.0, 0.5, 2000, max_norm, R.LR, R.B1, R.B2)
    assert abs(float(st["grad_norm"]) - total) <= 2 * U * total
    if coef == 1.0:
        assert float(st["clip_coef"]) == 1.0
    else:
        assert abs(float(st["clip_coef"]) - coef) <= 4 * U * coef
    assert R.same_bits(st["gscale"], (F(gs) / F(S)) * st["clip_coef"]).all()
    # no clipping: the coefficient is exactly 1; norm 0: max_norm / 1e-6 clamps to 1; infinite norm: found
    assert float(R.amp_update_ref(_state(S), 1e6, 0, gs, False, 2.0, 0.5, 2000, None, R.LR, R.B1, R.B2)["clip_coef"]) == 1.0
    z = R.amp_update_ref(_state(S), 0.0, 0, gs, False, 2.0, 0.5, 2000, max_norm, R.LR, R.B1, R.B2)
    assert (float(z["grad_norm"]), float(z["clip_coef"]), z["found_inf"]) == (0.0, 1.0, 0)
    i = R.amp_update_ref(_state(S, applied=4), math.inf, 0, gs, False, 2.0, 0.5, 2000, max_norm, R.LR, R.B1, R.B2)
    assert (i["found_inf"], i["applied_steps"], i["skipped_steps"], float(i["gscale"]), float(i["lr_over_bc1"])) == (1, 4, 1, -7.0, -8.0)
    assert R.amp_update_ref(_state(S), math.inf, 0, gs, False, 2.0, 0.5, 2000, None, R.LR, R.B1, R.B2)["found_inf"] == 0


def test_adam_scalars_and_the_large_t_rule():
    lr1, isb = R.adam_scalars(R.LR, R.B1, R.B2, 1)
    b1, b2 = float(F(R.B1)), float(F(R.B2))
    assert lr1 == F(float(F(R.LR)) / (1.0 - b1)) and isb == F(1.0 / math.sqrt(1.0 - b2))
    assert not R.bias_is_exactly_one(R.B2, 10 ** 4) and R.bias_is_exactly_one(R.B2, 10 ** 5) and R.bias_is_exactly_one(R.B2, 10 ** 7)
    assert 1.0 - math.pow(b2, 1e5) == 1.0 and 1.0 - math.pow(b2, 1e4) < 1.0
    assert 1.0 - math.pow(b1, 400.0) == 1.0 and R.bias_is_exactly_one(R.B1, 400) and not R.bias_is_exactly_one(R.B1, 300)
    assert R.adam_scalars(R.LR, R.B1, R.B2, 2 ** 31 + 6) == (F(R.LR), F(1.0))


def test_sum_partials_is_a_sum():
    rng = np.random.RandomState(2)
    ps = rng.randint(0, 1 << 20, R.AMP_PARTS).astype(F)
    assert R.sum_partials(ps) == float(ps.astype(np.int64).sum())
    x = rng.uniform(0, 1, R.AMP_PARTS).astype(F)
    assert abs(R.sum_partials(x) - math.fsum(x.astype(np.float64))) <= 1e-12 * math.fsum(x.astype(np.float64))
    ps[517] = np.inf
    assert R.sum_partials(ps) == math.inf


# ---------------------------------------------------------------------------------------------------------------- the mask
def test_mask_expansion_across_the_word_boundary():
    n = 4 * 67 - 1                                                          # 67 groups, the last one ragged: two words
    bits = [0] * 67
    for j in (0, 5, 63, 65, 66):
        bits[j] = 1
    words = np.array([(1 << 0) | (1 << 5) | (1 << 63), (1 << 1) | (1 << 2) | (1 << 40)], dtype=np.uint64)     # bit 104: unused, ignored
    want = [bool(bits[i // 4]) for i in range(n)]
    got = R.expand_mask(words, n)
    assert got.tolist() == want
    assert got[4 * 63:4 * 64].all() and not got[4 * 64:4 * 65].any() and got[4 * 65:4 * 66].all() and got[4 * 66:].tolist() == [True] * 3
    assert R.expand_mask(None, 5).tolist() == [True] * 5
    assert R.expand_mask(words.view(np.int64), n).tolist() == want          # the trainer hands the words over as int64
    for kind, groups in (("bit63", [63]), ("bit64", [64]), ("tail", [66]), ("ones", list(range(67)))):
        assert np.nonzero(R.expand_mask(R.mask_words(kind, n), n)[::4])[0].tolist() == groups, kind
    assert R.mask_words("null", n) is None and R.mask_words("ones", n)[1] == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert not R.expand_mask(R.mask_words("bit64", 8), 8).any() and not R.expand_mask(R.mask_words("bit63", 8), 8).any()
    r = R.expand_mask(R.mask_words("random", 4099), 4099)
    assert r.any() and not r.all()


# ---------------------------------------------------------------------------------------------------------------- stats_positions
def _walk(n):
    """k_grad_stats' two loops, restated literally over all lanes at once: for every float4 index, how often it is read and by
    which load ("a", "b", "c", "d" of the unrolled body, "r" of the remainder loop)."""
    n4, s = n >> 2, R.STRIDE
    reads = np.zeros(max(n4, 1), dtype=np.int64)
    path = np.full(max(n4, 1), "-", dtype="<U1")
    i = np.arange(s, dtype=np.int64)                                        # lane t starts at float4 t
    while True:
        go = i + 3 * s < n4
        if not go.any():
            break
        for k, name in enumerate("abcd"):
            idx = i[go] + k * s
            reads[idx] += 1
            path[idx] = name
        i = np.where(go, i + 4 * s, i)
    while True:
        go = i < n4
        if not go.any():
            break
        reads[i[go]] += 1
        path[i[go]] = "r"
        i = np.where(go, i + s, i)
    return reads[:n4], path[:n4]


@pytest.mark.parametrize("n4", [1, 257, R.STRIDE, 3 * R.STRIDE, 3 * R.STRIDE + 1, 4 * R.STRIDE - 1, 4 * R.STRIDE, 4 * R.STRIDE + 1,
                                7 * R.STRIDE + 5])
def test_stats_positions_against_a_literal_walk(n4):
    s = R.STRIDE
    for tail in R.STATS_TAILS:
        n = 4 * n4 + tail
        reads, path = _walk(n)
        assert (reads == 1).all()                                           # the loops themselves read every float4 once
        pos = R.stats_positions(n)
        assert len(set(pos)) == len(pos) and all(0 <= i < n for i in pos)
        assert [i for i in pos if i >= 4 * n4] == list(range(4 * n4, n))    # every tail element
        quads = sorted(set(i // 4 for i in pos if i < 4 * n4))
        assert all(4 * q in pos and 4 * q + 3 in pos for q in quads)
        # every kind of load the walk makes at this size is named, and so are the first and last float4
        assert set(path[quads]) == set(path), (n, set(path[quads]), set(path))
        assert quads[0] == 0 and quads[-1] == n4 - 1
    # the sizes on either side of the unrolled loop's condition i + 3*stride < n4
    if n4 == 3 * s:
        assert set(path) == {"r"}
    if n4 == 3 * s + 1:
        assert path[0] == "a" and path[3 * s] == "d" and path[1] == "r" and {4 * 3 * s, 4 * 3 * s + 3} <= set(pos)
    if n4 == 4 * s + 1:
        assert path[4 * s] == "r" and (path[:4 * s] != "r").all() and 4 * 4 * s in pos
    if n4 == 7 * s + 5:
        assert path[4 * s] == "a" and path[7 * s + 4] == "d" and path[7 * s + 5 - 1 - s] == "c" and path[4 * s + 5] == "r"
