"""The fp64 statements of tests/_prep_ref.py against fp64 autograd through a literal formulation (a convolution followed by
eval-mode F.batch_norm), the table builder against the alignment the kernels rely on, and the tests' tables against the branches of
k_wgrad_finalize / k_weight_prep they are meant to reach -- so that a wrong statement cannot bless a wrong kernel
(tests/test_gpu_prep_finalize.py).  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _prep_ref as R

EPS = 1e-5


def _close(a, b, what, rtol=1e-12):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= rtol * scale, "%s: off by %g of %g" % (what, float((a - b).abs().max()), scale)


def _split(total, parts, g):
    """`parts` fp64 arrays of mixed sign and magnitude that add up to `total` (the last one takes the remainder)."""
    out = [np.asarray(torch.randn(total.shape, generator=g, dtype=torch.float64)) * 2.0 ** (i % 5 - 2) for i in range(parts - 1)]
    out.append(total - sum(out) if out else total.copy())
    return np.stack(out)


def _autograd_case(cout, ksz, bn, stem, nsplit, seed):
    """One conv (+ eval-mode BN) in fp64: autograd's dW / dgamma / dbeta, and finalize_statement fed the exact G = dL/d(folded
    weight) and the channel sums of the upstream gradient, split arbitrarily into nsplit slabs / 4 * nsplit rows."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    cin = 32
    L = R.Layer(cout, cin, 7 if stem else ksz * ksz, bn, True, stem, nsplit)
    T = R.build_table([L], torch.float32)
    r = T["rows"][0]
    K, cp = r["K"], r["cout_pad"]
    if stem:
        W = rnd(cout, 7, 8, 4).requires_grad_(True)                         # the embedding; [:, :, :7, :3] is the logical [O,3,7,7]
        x = rnd(2, 3, 12, 11)
        conv = lambda Wt: F.conv2d(x, Wt[:, :, :7, :3].permute(0, 3, 1, 2), stride=2, padding=3)
    else:
        W = rnd(cout, ksz, ksz, cin).requires_grad_(True)                   # [Cout][kh][kw][Cin], the arena's layout
        x = rnd(2, cin, 6, 5)
        conv = lambda Wt: F.conv2d(x, Wt.permute(0, 3, 1, 2), padding=ksz // 2)
    gamma, beta = (rnd(cout) + 2.0).requires_grad_(True), rnd(cout).requires_grad_(True)
    mean, var = rnd(cout) * 0.3, torch.rand(cout, generator=g, dtype=torch.float64) + 0.5
    z = conv(W)
    y = F.batch_norm(z, mean, var, gamma, beta, False, 0.0, EPS) if bn else z
    gy = rnd(*y.shape)
    y.backward(gy)
    # what the device holds: G = gradient w.r.t. the FOLDED weight of the convolution alone, and the channel sums of gy
    Wf = ((gamma / torch.sqrt(var + EPS)).view(-1, 1, 1, 1) * W if bn else W).detach().clone().requires_grad_(True)
    conv(Wf).backward(gy)
    G = Wf.grad.reshape(cout, K).numpy().copy()
    if stem:
        G[:, ~R.stem_keep(K)] = R.POISON                                    # whatever the wgrad kernel left there
    params = np.full(T["size"]["params"], R.POISON)
    buffers = np.full(T["size"]["buffers"], R.POISON)
    params[r["w_off"]:r["w_off"] + cout * K] = W.detach().reshape(-1).numpy()
    if bn:
        params[r["gamma_off"]:r["gamma_off"] + cout] = gamma.detach().numpy()
        params[r["beta_off"]:r["beta_off"] + cout] = beta.detach().numpy()
        buffers[r["mean_off"]:r["mean_off"] + cout] = mean.numpy()
        buffers[r["var_off"]:r["var_off"] + cout] = var.numpy()
    slabs = np.full(T["size"]["slabs"], R.POISON)
    s = slabs[r["slab_off"]:r["slab_off"] + nsplit * cp * K].reshape(nsplit, cp, K)
    s[:, :cout] = _split(G, nsplit, g)
    gsum = np.full(T["size"]["gsum"], R.POISON)
    q = gsum[r["gsum_off"]:r["gsum_off"] + 4 * nsplit * cp].reshape(4 * nsplit, cp)
    q[:, :cout] = _split(gy.sum((0, 2, 3)).numpy(), 4 * nsplit, g)
    st = R.finalize_statement(r, params, buffers, slabs, gsum, EPS)
    return r, W, gamma, beta, st, (params, buffers)


@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("cout,ksz,nsplit", [(18, 1, 1), (18, 3, 5), (64, 1, 7), (64, 3, 2)])
def test_finalize_statement_is_autograd(cout, ksz, nsplit, bn):
    r, W, gamma, beta, st, _ = _autograd_case(cout, ksz, bn, False, nsplit, 10 * cout + ksz)
    assert r["cout_pad"] == (32 if cout == 18 else 64)
    _close(st["dW"], W.grad.reshape(cout, -1), "dW")
    assert st["n_dW"] == nsplit and bool((st["A_dW"] >= st["dW"].abs() * (1 - 1e-12)).all())
    if bn:
        _close(st["dbeta"], beta.grad, "dbeta")
        _close(st["dgamma"], gamma.grad, "dgamma")
        assert st["n_dbeta"] == 4 * nsplit and bool((st["A_dbeta"] >= st["dbeta"].abs() * (1 - 1e-12)).all())
        assert bool((st["A_dgamma"] >= st["dgamma"].abs() * (1 - 1e-12)).all())
    else:
        assert "dbeta" not in st and "dgamma" not in st


@pytest.mark.parametrize("bn", [True, False])
def test_finalize_statement_stem_is_autograd(bn):
    """The logical [O,3,7,7] weight embedded in [O,7,8,4]: the structural zeros get zero gradient whatever the slabs hold there."""
    r, W, gamma, beta, st, _ = _autograd_case(32, 7, bn, True, 3, 77)
    keep = torch.from_numpy(R.stem_keep(224))
    assert int(keep.sum()) == 7 * 7 * 3
    dW = st["dW"]
    assert float(dW[:, ~keep].abs().max()) == 0.0 and float(W.grad.reshape(32, 224)[:, ~keep].abs().max()) == 0.0
    _close(dW, W.grad.reshape(32, 224), "stem dW")
    if bn:
        _close(st["dbeta"], beta.grad, "stem dbeta")
        _close(st["dgamma"], gamma.grad, "stem dgamma")


@pytest.mark.parametrize("cout,ksz", [(18, 1), (64, 3)])
def test_weight_prep_statement_is_the_folded_conv(cout, ksz):
    """conv(x, wf) + shift == batch_norm(conv(x, W)) in fp64; wd is wf transposed; padded channels are zero."""
    r, W, gamma, beta, _, (params, buffers) = _autograd_case(cout, ksz, True, False, 1, 5)
    st = R.weight_prep_statement(r, params, buffers, EPS)
    cp, cin = r["cout_pad"], r["cin"]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, cin, 6, 5, generator=g, dtype=torch.float64)
    mean = torch.from_numpy(buffers[r["mean_off"]:r["mean_off"] + cout])
    var = torch.from_numpy(buffers[r["var_off"]:r["var_off"] + cout])
    want = F.batch_norm(F.conv2d(x, W.detach().permute(0, 3, 1, 2), padding=ksz // 2), mean, var, gamma.detach(), beta.detach(), False, 0.0, EPS)
    wf = st["wf"].reshape(cp, ksz, ksz, cin)
    got = F.conv2d(x, wf.permute(0, 3, 1, 2), padding=ksz // 2) + st["shift"].view(1, -1, 1, 1)
    _close(got[:, :cout], want, "folded conv")
    assert float(got[:, cout:].abs().max() if cp > cout else 0.0) == 0.0
    assert torch.equal(st["wd"], st["wf"].permute(2, 1, 0)) and st["wd"].shape == (cin, ksz * ksz, cp)
    assert float(st["scale"][cout:].abs().sum() + st["shift"][cout:].abs().sum()) == 0.0
    nobn = R.build_table([R.Layer(cout, cin, ksz * ksz, False)], torch.float32)["rows"][0]
    st2 = R.weight_prep_statement(nobn, params, buffers, EPS)
    assert torch.equal(st2["scale"][:cout], torch.ones(cout, dtype=torch.float64)) and float(st2["shift"].abs().max()) == 0.0
    assert torch.equal(st2["wf"][:cout].reshape(-1), W.detach().reshape(-1))


def test_weight_prep_fp8_statement():
    L = [R.Layer(18, 64, 1, True, True, False, 1, True), R.Layer(32, 64, 1, False, True, False, 1, True)]
    T = R.build_table(L, torch.float32)
    params, buffers = R.make_params(T, 3, zero_rows=((0, 2),))
    amax = R.make_amax(2)
    for i, r in enumerate(T["rows"]):
        st = R.weight_prep_fp8_statement(r, params, buffers, amax[i * 80:(i + 1) * 80], EPS)
        c, cp = r["cout"], r["cout_pad"]
        scaled = st["target"][:c] / st["wscale"][:c, None]
        peak = scaled.abs().max(1).values
        zero = torch.tensor([i == 0 and co == 2 for co in range(c)])
        assert bool((peak[~zero] - 448.0).abs().max() < 1e-9) and bool((peak[zero] == 0).all())
        assert bool((st["wscale"][:c][zero] == 1.0).all()) and float(st["wscale"][c:].abs().sum()) == 0.0 and float(st["target"][c:].abs().sum()) == 0.0
        if not r["bn"]:
            assert torch.equal(st["target"][:c].reshape(-1), torch.from_numpy(params[r["w_off"]:r["w_off"] + c * r["K"]].astype(np.float64)))
        blk = st["amax"]
        assert float(blk[64]) == 2.0 + i and float(blk[:64].abs().sum()) == 0.0 and bool((blk[65:] == R.CANARY_F).all())
    assert float(R.e4m3_spacing(torch.tensor([448.0, 256.0, 255.0, 1.0, 2.0 ** -6, 2.0 ** -7, 0.0], dtype=torch.float64)).sub(
        torch.tensor([32.0, 32.0, 16.0, 0.125, 2.0 ** -9, 2.0 ** -9, 2.0 ** -9], dtype=torch.float64)).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- tables
def _tables():
    out = [("finalize/" + c, R.finalize_layers(c)) for c in R.FINALIZE_CASES]
    out += [("1x1 x 256", R.many_1x1_layers(256)), ("1x1 x 257", R.many_1x1_layers(257)), ("prep", R.prep_layers()), ("fp8", list(R.FP8_LAYERS))]
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_build_table_alignment_and_gaps(dtype):
    for name, layers in _tables():
        T = R.build_table(layers, dtype)
        es = T["es"]
        for arena in T["own"]:
            m = R.owned_mask(T, arena)                                       # asserts that the owned ranges are disjoint
            assert not m.all() and not m[-1], "%s: %s has no unowned gap at its end" % (name, arena)
            edges = np.flatnonzero(np.diff(m.astype(np.int8)) == -1)
            if arena not in ("params", "buffers"):                           # every owned range is followed by a gap of its own
                assert len(edges) == len(T["own"][arena]), "%s: %s: ranges touch" % (name, arena)
        for r, L in zip(T["rows"], layers):
            assert r["w_off"] % 4 == 0 and r["slab_off"] % 4 == 0 and r["shift_off"] % 4 == 0 and r["gsum_off"] % 4 == 0     # 16-byte loads
            assert r["wfwd_off"] % 256 == 0 and (r["wdgrad_off"] % 256 == 0 if L.need_dgrad else (r["wdgrad_off"] == -1 and r["wd_reserved"] % 256 == 0))
            assert (r["w8_off"] % 256 == 0 and r["wscale_off"] % 4 == 0) if L.fp8 else (r["w8_off"] == -1 and r["wscale_off"] == -1)
            assert r["cout_pad"] % 32 == 0 and 0 <= r["cout_pad"] - r["cout"] < 32 and r["K"] % 32 == 0
            assert (r["gamma_off"] >= 0) == bool(L.bn) and all((r[k] >= 0) == bool(L.bn) for k in ("beta_off", "mean_off", "var_off"))
            assert len(R.conv_fields(r)) == 18
        # the image of a layer is followed by the next one exactly one rounded size + one gap later (backend_hip._layout + the gap)
        r0, r1 = T["rows"][0], T["rows"][1]
        assert r1["wfwd_off"] - r0["wfwd_off"] == 2 * (R._r256(r0["cout_pad"] * r0["K"] * es) + 256)
        assert r1["shift_off"] - r0["shift_off"] == 2 * r0["cout_pad"] + 4


def test_finalize_tables_reach_every_branch():
    """The census the GPU tests rely on: the selector of k_wgrad_finalize, mirrored in R.finalize_branch, sends the table's layers
    down every branch; every branch sees an nsplit below its unroll, an exact multiple of it and a multiple plus a tail."""
    want = {32: ("grouped", 32), 224: ("grouped", 4), 288: ("grouped", 3), 512: ("grouped", 2), 576: ("long", [1]), 1024: ("long", [1]),
            1152: ("long", [2]), 2304: ("long", [3]), 4608: ("long", [4, 1])}
    Ks = [L.taps * L.cin for L, _ in R.FINALIZE_LAYERS]
    assert Ks == sorted(want)
    census = set()
    for K in Ks:
        kind, v = R.finalize_branch(K)
        assert (kind, v) == want[K]
        census |= {"G>1"} if kind == "grouped" else {"ncol %d" % c for c in v} | ({"second kb round"} if len(v) > 1 else set())
        assert R.finalize_branch(K, grouped=False)[0] == "long"
        if K < 1024:
            assert R.finalize_branch(K, grouped=False) == ("long", [1])      # FINALIZE_GROUPS = 0: one column with idle lanes
    assert census == {"G>1", "ncol 1", "ncol 2", "ncol 3", "ncol 4", "second kb round"}
    assert 256 - 4 * (224 // 4) == 32 and 256 - 3 * (288 // 4) == 40 and 576 // 4 == 144 and 1024 // 4 == 256        # idle lanes / partial / full column
    for (L, ns), K in zip(R.FINALIZE_LAYERS, Ks):
        kind, v = R.finalize_branch(K)
        for u in R.finalize_unrolls(K):
            below, mult, tail = ns
            assert below < u and mult % u == 0 and tail > u and tail % u != 0, (K, u, ns)
        if kind == "grouped":
            assert set(ns) <= {1, v - 1, v + 1, 8 * v - 1, 8 * v, 9 * v + 1}
        else:
            assert set(ns) <= {1, 2, 3, 7, 8, 9, 17}
    for case in R.FINALIZE_CASES:
        layers = R.finalize_layers(case)
        assert all((L.cout + 31) // 32 * 32 == 32 for L in layers) and sum(L.cout == 18 for L in layers) == 2
        assert {bool(L.bn) for L in layers} == {True, False} and {bool(L.need_dgrad) for L in layers} == {True, False}
        assert sum(L.stem for L in layers) == 1
    bn_ns = [L.nsplit for c in R.FINALIZE_CASES for L in R.finalize_layers(c) if L.bn]
    assert any(4 * n > 256 for n in bn_ns) and any(4 * n < 64 for n in bn_ns)


def test_many_layer_tables():
    for n in (256, 257):
        layers = R.many_1x1_layers(n)
        assert len(layers) == n and all(L.taps * L.cin == 32 for L in layers)
        first = np.cumsum([0] + [L.cout for L in layers])
        assert set(np.diff(first).tolist()) == {18, 32} and len(set((first[1:] - first[:-1]).tolist())) == 2
        assert {bool(L.bn) for L in layers} == {True, False}


def test_prep_table_deals_twice_and_mixes():
    layers = R.prep_layers()
    assert 240 <= len(layers) <= 256
    assert R.prep_items(layers) > 2048, R.prep_items(layers)                 # the grid-stride loop of the 2048 workgroups trips twice
    assert {L.cin for L in layers} == {32, 64, 96} and {L.cout for L in layers} == {18, 32, 64, 96} and {L.taps for L in layers} == {1, 7, 9}
    assert sum(not L.bn for L in layers) >= 20 and sum(not L.need_dgrad for L in layers) >= 20 and sum(L.stem for L in layers) >= 5
    assert any(L.cin == 32 and L.bn and L.need_dgrad for L in layers) and any(L.cin == 96 and L.cout == 96 for L in layers)


def test_fp8_table():
    L = list(R.FP8_LAYERS)
    assert sorted({x.taps * x.cin for x in L if x.fp8}) == [64, 576, 1152, 4608]
    trips = {K: (K // 4 + 255) // 256 for K in (64, 576, 1152, 4608)}
    assert trips == {64: 1, 576: 1, 1152: 2, 4608: 5}
    assert sum(not x.fp8 for x in L) == 1 and any(not x.bn and x.fp8 for x in L) and any(x.cout == 18 for x in L)
    assert all(L[li].fp8 and row < L[li].cout for li, row in R.FP8_ZERO_ROWS)
    assert {0, 63} <= set(R.FP8_AMAX_SLOT[:len(L)]) and len(set(R.FP8_AMAX_SLOT[:len(L)])) == len(L)


def test_input_makers():
    T = R.build_table(R.finalize_layers("tail"), torch.float32)
    slabs, gsum = R.make_slabs(T, 1)
    for arena, a in (("slabs", slabs), ("gsum", gsum)):
        m = R.owned_mask(T, arena)
        assert bool((a[~m] == np.float32(R.POISON)).all())
    for r in T["rows"]:
        ns, cp, K, c = r["nsplit"], r["cout_pad"], r["K"], r["cout"]
        s = slabs[r["slab_off"]:r["slab_off"] + ns * cp * K].reshape(ns, cp, K)
        assert bool((s[:, c:] == np.float32(R.POISON)).all()) and float(np.abs(s[:, :c]).max()) <= 16.0
        assert bool((s[:, :c] > 0).any()) and bool((s[:, :c] < 0).any())
        mags = np.abs(s[:, :c]).reshape(ns, -1)
        lo, hi = mags.min(1), mags.max(1)
        assert bool((hi < 2 * lo).all())                                     # one binade per slab ...
        if ns >= 9:
            assert hi.max() / lo.min() >= 2.0 ** 4                           # ... spread over the slabs
        # ONE dropped slab moves every element by more than twice the bound of its sum
        st = R.finalize_statement(r, *R.make_params(T, 2), slabs, gsum)
        b = R.bound(st["n_G"], st["A_G"], st["G"])
        assert float((torch.from_numpy(mags.min(1).min().reshape(1).astype(np.float64)) / b.max())) > 2.0, (K, ns)
    p, b = R.make_params(T, 2)
    assert bool((p[~R.owned_mask(T, "params")] == np.float32(R.POISON)).all()) and bool((b[~R.owned_mask(T, "buffers")] == np.float32(R.POISON)).all())
    ss = R.make_ssarena(T, p, b)
    assert bool((ss[~R.owned_mask(T, "ssarena")] == np.float32(R.CANARY_F)).all()) and np.float32(R.CANARY_F) == R.CANARY_F
