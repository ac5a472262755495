"""dcf_weight_prep, dcf_weight_prep_fp8 and dcf_wgrad_finalize / dcf_wgrad_finalize_rows against the fp64 statements of
tests/_prep_ref.py, on tables built so that every branch of the kernels runs: the grouped short-row reduction (G = 32, 4, 3, 2), the
long-row branches (one column partial / full, two columns, the four-column branch with a column off, a second round of 1024
vectors), each with an nsplit below its unroll, an exact multiple of it and a multiple plus a tail; the stem's structural zeros; the
gsum loop beyond 256 rows; the rows form's binary search at 256 layers and its fall-back to the grid form at 257; the weight-prep
deal of > 2048 tile items over 2048 workgroups; the fp8 images, their per-row scales and the roll of the activation maxima.

Tolerances (none is a measured number):
  * a sum of n fp32 terms with absolute sum A, in any order: _fusion_ref.bound(n, A, want) = 1.01 * (n + 8) * 2^-24 * A (+ the storage
    rounding 0 / 2^-8 / 2^-11 of |want| for fp32 / bf16 / fp16 results);
  * a result that carries a folded-BN factor (scale = gamma * rsqrtf(var + eps), invstd): R.FACTOR * |want| = 8 * 2^-24 * |want| on top
    -- 0.5 ulp for the add, <= 2 ulp for the device rsqrtf, 0.5 ulp for the gamma product, 0.5 ulp for the final product: under 4 ulp
    of 2^-23.  (No ROCm math document ships with the toolchain this was written against; the public HIP math API table gives rsqrtf
    1 ulp, so 2 is on the safe side and the term was not widened.)
  * everything else is exact: padded rows, canaries, no-BN images, bitwise equality of the two finalisation forms, the fp8 bits of
    no-BN layers, the rolled maxima.
Every output arena is pre-filled with a canary (0xFF bytes / R.CANARY_F), so "zero" means "written as zero" and "untouched" can be
asserted; the padded rows of the slabs, the padded columns of gsum and every unowned input element hold 1e30."""
import functools

import numpy as np
import pytest
import torch

import _prep_ref as R
from _util import pkg

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": 0, "bf16": 1, "f16": 2}
BITS = {4: torch.int32, 2: torch.int16}


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


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _conv_table(T):
    H = pkg("_hip")
    tab = (H.ConvParam * len(T["rows"]))()
    for i, r in enumerate(T["rows"]):
        tab[i] = H.ConvParam(*R.conv_fields(r))
    return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()


def _f8_table(T):
    H = pkg("_hip")
    tab = (H.F8Param * len(T["rows"]))()
    for i, r in enumerate(T["rows"]):
        tab[i] = H.F8Param(r["w8_off"], r["wscale_off"])
    return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()


# ================================================================================================================== finalisation
class _Fin:
    """One finalisation table with its inputs on the host and on the device, and the statements of all layers."""

    def __init__(self, layers, seed):
        self.layers = layers
        self.T = T = R.build_table(layers, torch.float32)
        self.params, self.buffers = R.make_params(T, seed)
        self.slabs, self.gsum = R.make_slabs(T, seed + 1)
        self.ss = R.make_ssarena(T, self.params, self.buffers)
        self.st = [R.finalize_statement(r, self.params, self.buffers, self.slabs, self.gsum) for r in T["rows"]]
        self.written = R.owned_mask(T, "params")                 # W, gamma, beta of every layer: what finalisation writes in grads
        self.table = _conv_table(T)
        self.dev = [_dev(a) for a in (self.params, self.buffers, self.ss, self.slabs, self.gsum)]
        self.couts = np.array([L.cout for L in layers], dtype=np.int32)

    def run(self, form, slabs=None, gsum=None):
        """One launch onto a canary-filled gradient arena; returns it as a numpy array."""
        H = pkg("_hip")
        p, b, ss, sl, gs = self.dev
        sl = sl if slabs is None else slabs
        gs = gs if gsum is None else gsum
        grads = torch.full((self.T["size"]["params"],), R.CANARY_F, dtype=torch.float32, device="cuda")
        n = len(self.layers)
        if form == "grid":
            H.call("dcf_wgrad_finalize", self.table, n, int(self.couts.max()), p, b, ss, sl, gs, grads, R.EPS, H.stream_ptr())
        else:
            H.call("dcf_wgrad_finalize_rows", self.table, n, self.couts, p, b, ss, sl, gs, grads, R.EPS, H.stream_ptr())
        torch.cuda.synchronize()
        return grads.cpu().numpy()

    def check(self, grads, what):
        """Every layer's dW, dbeta, dgamma within its bound of the statement; everything else in grads still the canary."""
        assert bool((grads[~self.written] == np.float32(R.CANARY_F)).all()), "%s: %d elements outside the layers' ranges written" % (
            what, int((grads[~self.written] != np.float32(R.CANARY_F)).sum()))
        quiet = len(self.layers) > 16
        for i, (r, st) in enumerate(zip(self.T["rows"], self.st)):
            c, K = r["cout"], r["K"]
            tag = "%s layer %d (K %d, nsplit %d)" % (what, i, K, r["nsplit"])
            dW = torch.from_numpy(grads[r["w_off"]:r["w_off"] + c * K].reshape(c, K))
            if quiet:
                ok = lambda got, want, allowed: bool(((got.double() - want).abs() <= allowed).all())
            if not r["bn"]:
                if quiet:
                    assert ok(dW, st["dW"], R.bound(st["n_dW"], st["A_dW"], st["dW"])), tag
                else:
                    R.assert_within(dW, st["dW"], st["n_dW"], st["A_dW"], torch.float32, tag + " dW")
                continue
            db = torch.from_numpy(grads[r["beta_off"]:r["beta_off"] + c])
            dg = torch.from_numpy(grads[r["gamma_off"]:r["gamma_off"] + c])
            a_dW = R.bound(st["n_dW"], st["A_dW"], st["dW"]) + R.factor_term(st["dW"])
            a_dg = R.bound(st["n_dgamma"], st["A_dgamma"], st["dgamma"]) + R.factor_term(st["dgamma"])
            if quiet:
                assert ok(dW, st["dW"], a_dW) and ok(dg, st["dgamma"], a_dg), tag
                assert ok(db, st["dbeta"], R.bound(st["n_dbeta"], st["A_dbeta"], st["dbeta"])), tag
            else:
                R.assert_allowed(dW, st["dW"], a_dW, tag + " dW")
                R.assert_within(db, st["dbeta"], st["n_dbeta"], st["A_dbeta"], torch.float32, tag + " dbeta")
                R.assert_allowed(dg, st["dgamma"], a_dg, tag + " dgamma")
            if r["flags"] & 1:
                assert float(dW[:, torch.from_numpy(~R.stem_keep(K))].abs().max()) == 0.0, tag + ": structural zeros of the stem"


@functools.lru_cache(maxsize=None)
def _fin(case):
    return _Fin(R.finalize_layers(case), 40 + R.FINALIZE_CASES.index(case))


@functools.lru_cache(maxsize=None)
def _fin_many(n):
    return _Fin(R.many_1x1_layers(n), 60 + n)


@functools.lru_cache(maxsize=None)
def _fin_grid(case):
    return _fin(case).run("grid")


@pytest.mark.parametrize("case", R.FINALIZE_CASES)
def test_finalize_grid_form(case):
    """dcf_wgrad_finalize on the nine-branch table: bounds, canaries, and the same bits from a second launch and from a launch whose
    padded slab rows / gsum columns / gaps hold 0 instead of 1e30."""
    f = _fin(case)
    got = _fin_grid(case)
    f.check(got, "grid/" + case)
    assert np.array_equal(f.run("grid").view(np.int32), got.view(np.int32)), "two launches differ"
    sl0, gs0 = R.make_slabs(f.T, 41 + R.FINALIZE_CASES.index(case), poison=0.0)
    m = f.slabs != np.float32(R.POISON)                          # the rows co < cout: the same values; everything else 0 for 1e30
    assert not m.all() and np.array_equal(sl0[m].view(np.int32), f.slabs[m].view(np.int32)) and float(np.abs(sl0[~m]).max()) == 0.0
    assert np.array_equal(f.run("grid", _dev(sl0), _dev(gs0)).view(np.int32), got.view(np.int32)), "the padding reaches a result"


@pytest.mark.parametrize("case", R.FINALIZE_CASES)
def test_finalize_rows_form_is_bitwise_the_grid_form(case):
    """dcf_wgrad_finalize_rows -- the form the product launches: one workgroup per (layer, row) found by binary search over the layers'
    first rows (18, 50, 68, ... here) -- gives the grid form's bits, twice, and leaves the same canaries."""
    f = _fin(case)
    got = f.run("rows")
    assert np.array_equal(got.view(np.int32), _fin_grid(case).view(np.int32))
    assert np.array_equal(f.run("rows").view(np.int32), got.view(np.int32)), "two launches differ"
    f.check(got, "rows/" + case)


@pytest.mark.parametrize("case", R.FINALIZE_CASES)
def test_finalize_groups_off(case, set_opt):
    """FINALIZE_GROUPS = 0: every short row goes down the one-column branch with idle lanes; same statement, same bounds."""
    grouped = _fin_grid(case)
    set_opt("FINALIZE_GROUPS", 0)
    f = _fin(case)
    for form in ("grid", "rows"):
        got = f.run(form)
        f.check(got, "groups off/%s/%s" % (form, case))
        # the option reached the kernel: slab order s0, s1, ... instead of group sums (s0 + sG + ...) + (s1 + ...) + ... rounds differently
        assert not np.array_equal(got.view(np.int32), grouped.view(np.int32)), "FINALIZE_GROUPS = 0 gave the grouped branch's bits"


def test_finalize_rows_257_layers_falls_back_to_the_grid_form():
    """One layer more than the rows form's kernel-argument table holds: the call must still be correct (it launches the grid form)."""
    f = _fin_many(257)
    grid, rows = f.run("grid"), f.run("rows")
    f.check(grid, "257 layers/grid")
    f.check(rows, "257 layers/rows")
    assert np.array_equal(grid.view(np.int32), rows.view(np.int32))


def test_finalize_rows_256_layers_irregular_first_rows():
    """The largest table the rows form takes itself: 8 steps of binary search over first rows that advance by 18 and 32 in turn."""
    f = _fin_many(256)
    first = np.concatenate([[0], np.cumsum(f.couts)])
    assert len(set(np.diff(first).tolist())) == 2 and int(first[-1]) == 128 * (18 + 32)
    rows = f.run("rows")
    f.check(rows, "256 layers/rows")
    assert np.array_equal(f.run("grid").view(np.int32), rows.view(np.int32))


# ================================================================================================================== weight prep
@functools.lru_cache(maxsize=None)
def _prep_inputs():
    layers = R.prep_layers()
    T = R.build_table(layers, torch.float32)                     # params / buffers offsets do not depend on the compute dtype
    params, buffers = R.make_params(T, 7)
    st = [R.weight_prep_statement(r, params, buffers) for r in T["rows"]]
    return layers, params, buffers, st


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_weight_prep(dtype):
    """250 layers, > 2048 (layer, tap, 64 x 64 tile) items dealt over 2048 workgroups: both images, scale and shift of every layer
    against the statement; padded rows / channels written as zero; wd bitwise the transpose of wf; no-BN images exactly the cast of W;
    every byte outside the images -- the reserved wd range of the layers with wdgrad_off = -1 included -- still the canary."""
    H = pkg("_hip")
    layers, params, buffers, sts = _prep_inputs()
    assert R.prep_items(layers) > 2048 and len(layers) <= 256
    td = TDT[dtype]
    T = R.build_table(layers, td)
    es = T["es"]
    warena = torch.full((T["size"]["warena"],), R.CANARY_B, dtype=torch.uint8, device="cuda")
    ss = torch.full((T["size"]["ssarena"],), R.CANARY_F, dtype=torch.float32, device="cuda")
    H.call("dcf_weight_prep", CODE[dtype], _conv_table(T), len(layers), _dev(params), _dev(buffers), warena, ss, R.EPS, H.stream_ptr())
    torch.cuda.synchronize()
    wa, ssc = warena.cpu(), ss.cpu().double()
    assert bool((wa[torch.from_numpy(~R.owned_mask(T, "warena"))] == R.CANARY_B).all()), "bytes outside the images written"
    assert bool((ssc[torch.from_numpy(~R.owned_mask(T, "ssarena"))] == R.CANARY_F).all()), "ssarena gaps written"
    worst = {"wf": 0.0, "scale": 0.0, "shift": 0.0}
    for i, (r, st) in enumerate(zip(T["rows"], sts)):
        c, cp, K, taps, cin = r["cout"], r["cout_pad"], r["K"], r["taps"], r["cin"]
        tag = "%s layer %d (cout %d, cin %d, taps %d, bn %d)" % (dtype, i, c, cin, taps, r["bn"])
        n = cp * K * es
        wf_raw = wa[r["wfwd_off"]:r["wfwd_off"] + n].view(td).reshape(cp, taps, cin)
        wf_bits = wf_raw.view(BITS[es])
        want = st["wf"]
        if dtype == "f16":
            assert bool(((want == 0) | (want.abs() >= 2.0 ** -14)).all()), tag + ": an fp16 image value in the subnormal range"
        assert int(wf_bits[c:].abs().max() if cp > c else 0) == 0, tag + ": padded rows of wf are not written as zero"
        scale, shift = ssc[r["shift_off"]:r["shift_off"] + cp], ssc[r["shift_off"] + cp:r["shift_off"] + 2 * cp]
        assert float(scale[c:].abs().sum() + shift[c:].abs().sum()) == 0.0, tag + ": scale / shift of padded channels"
        if r["bn"]:
            err = (wf_raw.double() - want).abs() - (R.STORE_ULP[td] + R.FACTOR) * want.abs()
            assert float(err.max()) <= 0, "%s: wf %.3g beyond one storage rounding + the factor term" % (tag, float(err.max()))
            worst["wf"] = max(worst["wf"], float(((wf_raw.double() - want).abs() / want.abs().clamp(min=1e-30)).max()))
            e_sc = (scale - st["scale"]).abs() - R.factor_term(st["scale"])
            e_sh = (shift - st["shift"]).abs() - (R.bound(2, st["A_shift"], st["shift"]) + R.factor_term(st["shift"]))
            assert float(e_sc.max()) <= 0 and float(e_sh.max()) <= 0, "%s: scale %.3g / shift %.3g beyond the bound" % (tag, float(e_sc.max()), float(e_sh.max()))
            worst["scale"] = max(worst["scale"], float(((scale - st["scale"]).abs() / st["scale"].abs().clamp(min=1e-30))[:c].max()))
            worst["shift"] = max(worst["shift"], float((shift - st["shift"]).abs().max()))
        else:
            W = torch.from_numpy(params[r["w_off"]:r["w_off"] + c * K]).reshape(c, taps, cin)
            assert torch.equal(wf_bits[:c], W.to(td).view(BITS[es])), tag + ": the no-BN image is not the cast of W"
            assert torch.equal(scale[:c], torch.ones(c, dtype=torch.float64)) and float(shift.abs().sum()) == 0.0, tag
        if r["wdgrad_off"] >= 0:
            wd_bits = wa[r["wdgrad_off"]:r["wdgrad_off"] + n].view(BITS[es]).reshape(cin, taps, cp)
            assert torch.equal(wd_bits, wf_bits.permute(2, 1, 0)), tag + ": wd is not the transpose of wf"
        else:
            lo = r["wd_reserved"]
            assert bool((wa[lo:lo + n] == R.CANARY_B).all()), tag + ": wdgrad_off = -1 but the reserved range was written"
    print("%s: worst relative error wf %.3g, scale %.3g; worst |shift error| %.3g" % (dtype, worst["wf"], worst["scale"], worst["shift"]))


def test_weight_prep_refuses_257_layers():
    """k_weight_prep keeps the layers' prefix sums in 257 LDS words: a longer table is an error, and nothing is written."""
    H = pkg("_hip")
    layers = R.prep_layers(257)
    T = R.build_table(layers, torch.bfloat16)
    params, buffers = R.make_params(T, 8)
    warena = torch.full((T["size"]["warena"],), R.CANARY_B, dtype=torch.uint8, device="cuda")
    ss = torch.full((T["size"]["ssarena"],), R.CANARY_F, dtype=torch.float32, device="cuda")
    with pytest.raises(H.DcfError):
        H.call("dcf_weight_prep", 1, _conv_table(T), 257, _dev(params), _dev(buffers), warena, ss, R.EPS, H.stream_ptr())
    torch.cuda.synchronize()
    assert bool((warena == R.CANARY_B).all()) and bool((ss == R.CANARY_F).all())


# ================================================================================================================== fp8 weight prep
def _f8_bits(x32):
    """e4m3 bits of an fp32 numpy array the way the kernel forms them: clamp to +-448, round to nearest even."""
    t = torch.from_numpy(np.clip(x32, np.float32(-448), np.float32(448)).astype(np.float32))
    return t.to(torch.float8_e4m3fn).view(torch.uint8)


def test_weight_prep_fp8():
    """Eight layers: K = 64 / 576 / 1152 / 4608 (1, 1, 2 and 5 trips of the 256-lane loop), one off the fp8 path, two without BN, two
    with cout 18, all-zero rows under a negative and a positive BN scale and without BN; the grid is 64 wide, so the 32-wide layers
    see workgroups beyond their cout_pad.
    No BN: bits and wscale exactly what numpy forms in fp32 the way the kernel does (am = max|W|, sw = 448 / am, v * sw).
    BN: wscale within the factor term; every element within half an e4m3 spacing (at |bn W| / wscale, times wscale) plus the factor
    term of bn * W -- the device's own bn cancels between the scaled value and wscale, what is left is the rsqrtf / product error of
    bn itself and the roundings of sw, bn * sw, v * m and am / 448; each row's maximum decodes to exactly +-448.
    An all-zero row must hold zero BITS: 0 * (negative bn) is -0, which the kernel wrote as 0x80 before this test existed."""
    H = pkg("_hip")
    layers = list(R.FP8_LAYERS)
    T = R.build_table(layers, torch.bfloat16)
    params, buffers = R.make_params(T, 9, zero_rows=R.FP8_ZERO_ROWS)
    r3 = T["rows"][3]                                              # the all-zero rows of the BN layer: one negative, one positive gamma
    params[r3["gamma_off"] + 0] = -abs(params[r3["gamma_off"] + 0])
    params[r3["gamma_off"] + 17] = abs(params[r3["gamma_off"] + 17])
    amax0 = R.make_amax(len(layers))
    w8 = torch.full((T["size"]["w8arena"],), R.CANARY_B, dtype=torch.uint8, device="cuda")
    ws = torch.full((T["size"]["wsarena"],), R.CANARY_F, dtype=torch.float32, device="cuda")
    amax = _dev(amax0)
    max_cp = max(r["cout_pad"] for r in T["rows"])
    assert max_cp == 64 and any(r["cout_pad"] == 32 for r in T["rows"])       # narrower layers see workgroups beyond their cout_pad
    H.call("dcf_weight_prep_fp8", _conv_table(T), _f8_table(T), len(layers), max_cp, _dev(params), _dev(buffers), w8, ws, amax, R.EPS,
           H.stream_ptr())
    torch.cuda.synchronize()
    w8c, wsc, am = w8.cpu(), ws.cpu(), amax.cpu().numpy().reshape(len(layers), R.F8_AMAX_STRIDE)
    assert bool((w8c[torch.from_numpy(~R.owned_mask(T, "w8arena"))] == R.CANARY_B).all()), "bytes outside the fp8 images written"
    assert bool((wsc[torch.from_numpy(~R.owned_mask(T, "wsarena"))] == R.CANARY_F).all()), "wsarena gaps written"
    zero_rows = set(R.FP8_ZERO_ROWS)
    for i, r in enumerate(T["rows"]):
        tag = "fp8 layer %d" % i
        blk0 = amax0.reshape(len(layers), R.F8_AMAX_STRIDE)[i]
        if r["w8_off"] < 0:
            assert np.array_equal(am[i].view(np.int32), blk0.view(np.int32)), tag + ": the amax block of a layer off the fp8 path changed"
            continue
        c, cp, K = r["cout"], r["cout_pad"], r["K"]
        st = R.weight_prep_fp8_statement(r, params, buffers, blk0)
        assert np.array_equal(am[i].astype(np.float64), st["amax"].numpy()), tag + ": amax roll"
        assert float(am[i, 64]) == 2.0 + i and R.FP8_AMAX_SLOT[i] == int(np.argmax(blk0[:64]))
        bits = w8c[r["w8_off"]:r["w8_off"] + cp * K].reshape(cp, K)
        wscale = wsc[r["wscale_off"]:r["wscale_off"] + cp]
        assert int(bits[c:].max() if cp > c else 0) == 0 and float(wscale[c:].abs().sum()) == 0.0, tag + ": padded rows"
        for li, row in zero_rows:
            if li == i:
                assert int(bits[row].max()) == 0 and float(wscale[row]) == 1.0, "%s: all-zero row %d: bits %#x, wscale %g" % (
                    tag, row, int(bits[row].max()), float(wscale[row]))
        W32 = params[r["w_off"]:r["w_off"] + c * K].reshape(c, K)
        if not r["bn"]:
            a = np.abs(W32).max(1) * np.float32(1.0)
            sw = np.where(a > 0, np.float32(448.0) / np.where(a > 0, a, np.float32(1.0)), np.float32(1.0)).astype(np.float32)
            m = np.float32(1.0) * sw
            prod = W32 * m[:, None]
            assert prod.dtype == np.float32
            assert torch.equal(bits[:c], _f8_bits(prod)), tag + ": no-BN bits are not the e4m3 conversion of the fp32 product"
            want_ws = np.where(a > 0, a / np.float32(448.0), np.float32(1.0)).astype(np.float32)
            assert np.array_equal(wscale[:c].numpy().view(np.int32), want_ws.view(np.int32)), tag + ": no-BN wscale is not am / 448 in fp32"
            continue
        live = torch.tensor([(i, row) not in zero_rows for row in range(c)])
        want_ws, target = st["wscale"][:c], st["target"][:c]
        e_ws = (wscale[:c].double() - want_ws).abs() - R.factor_term(want_ws)
        assert float(e_ws[live].max()) <= 0, "%s: wscale %.3g beyond the factor term" % (tag, float(e_ws[live].max()))
        deq = bits[:c].view(torch.float8_e4m3fn).double()
        allowed = 0.5 * R.e4m3_spacing(target.abs() / want_ws[:, None]) * want_ws[:, None] + R.factor_term(target)
        err = (deq * wscale[:c].double()[:, None] - target).abs() - allowed
        print("%s: largest excess over the fp8 bound %.3g" % (tag, float(err[live].max())))
        assert float(err[live].max()) <= 0, "%s: %d elements beyond half an e4m3 spacing + the factor term" % (tag, int((err[live] > 0).sum()))
        peak = target.abs().argmax(1)
        got_peak = deq[torch.arange(c), peak]
        assert torch.equal(got_peak[live], 448.0 * torch.sign(target[torch.arange(c), peak])[live]), tag + ": a row's maximum does not decode to +-448"
