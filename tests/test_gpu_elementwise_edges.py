"""The HBM-bound kernels between the convolutions (csrc/elementwise.hip: layout conversion, cast, ReLU backward + channel sums, the
fc2 bias under the neighbour sum, bilinear resize) against the statements of tests/_elementwise_ref.py at the smallest shapes at
which they can still go wrong.

Layout, cast and the masked ReLU gradient are compared BIT FOR BIT (a NaN equals any NaN; the sign of a zero counts).  Every sum is
compared with tests/_fusion_ref.py::bound(): an fp32 sum of n terms with absolute sum A lies within
1.01 * (n + 8) * 2^-24 * A + ulp_store * |want| of the fp64 value; n and A come from the statement.  No bound here is a bare tolerance.

The channel-sum kernels walk the tensor with a grid of up to 256 k threads; CHANSUM_KTHREADS = 1 caps it at 1024, so that tensors
of a few thousand pixels reach every loop of the walk (the two- and four-per-trip bodies, their tails, a last workgroup with idle
threads, workgroups whose first thread is not in channel group 0).

Resize: a result must be within the bound of the unfused statement at every element or of the fused one at every element
(R.assert_one_variant).  fp16 results: the storage term of the bound is relative, so the fp16 cases use inputs whose stored results
are zero or at least 2^-14 (positive inputs; the backward's upstream gradient scaled by a power of two chosen from the statement)."""
import functools
import os

import numpy as np
import pytest
import torch

import _elementwise_ref as R
from _util import GOLD, pkg, q, rnd
from test_gpu_elementwise import _post_relu

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
LAYOUT_C = (4, 8, 12, 36)                        # 8- and 4-channel vectors
LAYOUT_HW = ((1, 1), (3, 5), (17, 16))           # 17 x 16 x 2 = 544 pixels: three workgroups, the last one partly idle
RELU_C = (4, 8, 12, 24, 64)                      # channel groups 1, 1, 3, 3, 8
TRIPS = (1, 2, 3, 4, 5, 8, 9)                    # nvec / stride just below, at and just above these
INIT = 0.25                                      # what the accumulated-onto buffers hold on entry
CAST_PAIRS = (("f32", "bf16"), ("bf16", "f32"), ("f32", "f32"), ("bf16", "bf16"), ("f32", "f16"), ("f16", "f32"), ("f16", "f16"))
PARENT_FIXTURE = os.path.join(GOLD, "resize_bwd_parent.npz")


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


def _census_complete(x, what):
    c = R.table_census(x)
    assert all(v >= 1 for v in c.values()), "%s: the table is not all there: %r" % (what, c)


# ------------------------------------------------------------------------------------------------------------------ layout and cast
@pytest.mark.parametrize("C", LAYOUT_C)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nchw_to_nhwc_bits(dtype, C):
    ops, td = pkg("ops"), R.TDT[dtype]
    for i, hw in enumerate(LAYOUT_HW):
        x = R.table_tensor((2, C) + hw, 10 * C + i)
        if x.numel() >= 2 * len(R.value_table()):
            _census_complete(x, "nchw_to_nhwc input")
        got = ops.nchw_to_nhwc(x.cuda(), R.CODE[dtype])
        R.same_bits(got, R.nchw_to_nhwc_statement(x, td), "nchw_to_nhwc %s C=%d %r" % (dtype, C, hw))


@pytest.mark.parametrize("C", LAYOUT_C)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nhwc_to_nchw_bits(dtype, C):
    ops, td = pkg("ops"), R.TDT[dtype]
    for i, hw in enumerate(LAYOUT_HW):
        x32 = R.table_tensor((2,) + hw + (C,), 20 * C + i)
        if x32.numel() >= 2 * len(R.value_table()):
            _census_complete(x32, "nhwc_to_nchw input")
        x = x32.to(td)
        got = ops.nhwc_to_nchw(x.cuda(), R.CODE[dtype])
        assert got.dtype == torch.float32
        R.same_bits(got, R.nhwc_to_nchw_statement(x), "nhwc_to_nchw %s C=%d %r" % (dtype, C, hw))


@pytest.mark.parametrize("C", LAYOUT_C)
def test_layout_round_trip_f32(C):
    """nhwc_to_nchw(nchw_to_nhwc(x)) is x, bit for bit (a NaN stays a NaN)."""
    ops = pkg("ops")
    for i, hw in enumerate(LAYOUT_HW):
        x = R.table_tensor((2, C) + hw, 30 * C + i)
        R.same_bits(ops.nhwc_to_nchw(ops.nchw_to_nhwc(x.cuda(), 0), 0), x, "round trip C=%d %r" % (C, hw))


@pytest.mark.parametrize("pair", CAST_PAIRS, ids=["%s_to_%s" % p for p in CAST_PAIRS])
def test_cast_bits(pair):
    ops = pkg("ops")
    src_dt, dst_dt = pair
    for n in (4, 1020, 1028):                                   # one vector; four workgroups less / plus one vector of 1024
        x32 = R.table_tensor((n,), n + len(src_dt))
        if n >= 1020:
            _census_complete(x32, "cast input")
        src = x32.to(R.TDT[src_dt])
        got = ops.cast(src.cuda(), R.CODE[dst_dt])
        assert got.dtype == R.TDT[dst_dt]
        R.same_bits(got, R.cast_statement(src, R.TDT[dst_dt]), "cast %s -> %s n=%d" % (src_dt, dst_dt, n))


def test_cast_rejects_what_it_cannot_do():
    ops, H = pkg("ops"), pkg("_hip")
    for src_dt, dst_dt in (("bf16", "f16"), ("f16", "bf16")):
        with pytest.raises(H.DcfError):
            ops.cast(torch.zeros(8, dtype=R.TDT[src_dt], device="cuda"), R.CODE[dst_dt])
    for n in (1, 6, 1023):
        with pytest.raises(H.DcfError):
            ops.cast(torch.zeros(n, device="cuda"), 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_image_to_nhwc4_bits(dtype):
    """uint8 [B,3,H,W] -> x / 255 in [B,H+6,W+8,4]: the interior bit for bit, every halo / pitch / fourth-channel element +0.0."""
    ops, td = pkg("ops"), R.TDT[dtype]
    for (Hh, W) in ((1, 1), (5, 3), (16, 8)):
        g = torch.Generator().manual_seed(Hh)
        img = torch.randint(0, 256, (2, 3, Hh, W), generator=g, dtype=torch.int64).to(torch.uint8)
        k = min(256, img.numel())
        flat = img.view(-1)
        flat[torch.randperm(img.numel(), generator=g)[:k]] = torch.arange(255, 255 - k, -1).to(torch.uint8)      # 255, 254, ... first
        if img.numel() >= 256:
            assert len(set(flat.tolist())) == 256, "not all 256 byte values are in the image"
        else:
            assert int(flat.max()) == 255 and len(set(flat.tolist())) >= min(k, 6)
        y = torch.full((2, Hh + 6, W + 8, 4), float("nan"), dtype=td, device="cuda")
        pkg("_hip").call("dcf_image_to_nhwc4", R.CODE[dtype], img.cuda(), y, 2, Hh, W, pkg("_hip").stream_ptr())   # into a poisoned buffer
        want = R.image_statement(img, td)
        R.same_bits(y, want, "image_to_nhwc4 %s %dx%d" % (dtype, Hh, W))
        R.same_bits(ops.image_to_nhwc4(img.cuda(), R.CODE[dtype]), want, "ops.image_to_nhwc4 %s %dx%d" % (dtype, Hh, W))
        assert int(R.bits(y)[~R.image_interior_mask(2, Hh, W)].abs().sum()) == 0


# ------------------------------------------------------------------------------------------------------------------ ReLU family
def _npix_list(C):
    V, cg, _, stride = R.chan_stride(10 ** 6, C, 1)
    assert stride == (1023 if cg == 3 else 1024)
    per = stride // cg                                           # pixels per trip of the whole grid
    return [k * per + d for k in TRIPS for d in (-1, 0, 1)]


@functools.lru_cache(maxsize=None)
def _relu_inputs(npix, C, dtype):
    """(y, gy [npix,C] in the storage type, cnt fp32 [npix]) on the CPU.  y: the pool tests' post-ReLU generator (about 60 % exact
    zeros, a channel all zero, one constant) with -0.0 and the smallest positive subnormal of the storage type planted; cnt in
    0..3 with a whole run of zeros."""
    td = R.TDT[dtype]
    y = _post_relu((1, C, npix, 1), 7 + npix % 5, R.CODE[dtype])[0, :, :, 0].t().contiguous().to(td)
    flat = y.view(-1)
    flat[0::11] = torch.tensor(-0.0).to(td)
    flat[5::11] = torch.tensor(R.SMALLEST_SUBNORMAL[td], dtype=torch.float64).to(td)
    neg_zero = int(R.bits(torch.tensor(-0.0).to(td)))
    assert int((R.bits(y) == neg_zero).sum()) >= 1 and int((y.double() == R.SMALLEST_SUBNORMAL[td]).sum()) >= 1
    assert float((y == 0).float().mean()) >= 0.3, "too few exact zeros in y"
    gy = q(rnd((npix, C), 40 + npix % 7), R.CODE[dtype]).to(td)
    g = torch.Generator().manual_seed(npix)
    cnt = torch.randint(0, 4, (npix,), generator=g).float()
    cnt[npix // 3:npix // 3 + max(1, npix // 5)] = 0.0
    assert int(cnt.max()) <= 3 and (npix < 40 or int((cnt == 3).sum()) > 0)
    return y, gy, cnt


def _relu_cases(C):
    return [(n, True) for n in _npix_list(C)] + [(37, False)]    # (npix, CHANSUM_KTHREADS = 1?): the last one is a single trip


def _sums(got, g, cnt, what):
    want, n, A = R.chansum_statement(g.float(), cnt, INIT)
    R.assert_within(got, want, n, A, torch.float32, what)


@pytest.mark.parametrize("C", RELU_C)
@pytest.mark.parametrize("dtype", DTYPES)
def test_relu_bwd_chansum_edges(dtype, C, set_opt):
    ops, code = pkg("ops"), R.CODE[dtype]
    for npix, capped in _relu_cases(C):
        set_opt("CHANSUM_KTHREADS", 1 if capped else None)
        what = "relu_bwd_chansum %s C=%d npix=%d" % (dtype, C, npix)
        y, gy, _ = _relu_inputs(npix, C, dtype)
        want = R.relu_mask_statement(gy, y)
        yd = y.cuda()
        gd, gsum = gy.cuda(), torch.full((C,), INIT, device="cuda")
        ops.relu_bwd_chansum(code, gd, yd, gsum, True)
        R.same_bits(gd, want, what)
        _sums(gsum, want, None, what + " sums")
        g2 = gy.cuda()
        ops.relu_bwd_chansum(code, g2, yd, None, True)                       # no sum buffer: the mask alone
        R.same_bits(g2, want, what + " gsum=None")
        g3, gsum3 = gy.cuda(), torch.full((C,), INIT, device="cuda")
        ops.relu_bwd_chansum(code, g3, None, gsum3, False)                   # no ReLU: the tensor is only read
        assert torch.equal(R.bits(g3), R.bits(gy)), what + " relu=False wrote the tensor"
        _sums(gsum3, gy, None, what + " relu=False sums")


@pytest.mark.parametrize("C", RELU_C)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rowscale_bias_bwd_edges(dtype, C, set_opt):
    ops, code = pkg("ops"), R.CODE[dtype]
    for npix, capped in _relu_cases(C):
        set_opt("CHANSUM_KTHREADS", 1 if capped else None)
        what = "rowscale_bias_bwd %s C=%d npix=%d" % (dtype, C, npix)
        _, gy, cnt = _relu_inputs(npix, C, dtype)
        gd, gb = gy.cuda(), torch.full((C,), INIT, device="cuda")
        ops.rowscale_bias_bwd(code, gd, cnt.cuda(), gb)
        assert torch.equal(R.bits(gd), R.bits(gy)), what + " wrote gy"
        _sums(gb, gy, cnt, what)


@pytest.mark.parametrize("C", RELU_C)
@pytest.mark.parametrize("dtype", DTYPES)
def test_relu_mask_rowscale_bwd_edges(dtype, C, set_opt):
    """One pass: the masked gradient in a tensor of its own, bit-equal to the statement and to the in-place route; gy untouched;
    gb2 += the cnt-weighted sums of the UNMASKED gradient."""
    ops, code = pkg("ops"), R.CODE[dtype]
    for npix, capped in _relu_cases(C):
        set_opt("CHANSUM_KTHREADS", 1 if capped else None)
        what = "relu_mask_rowscale_bwd %s C=%d npix=%d" % (dtype, C, npix)
        y, gy, cnt = _relu_inputs(npix, C, dtype)
        gd, yd, gb = gy.cuda(), y.cuda(), torch.full((C,), INIT, device="cuda")
        gout = ops.relu_mask_rowscale_bwd(code, gd, yd, cnt.cuda(), gb)
        assert gout.data_ptr() != gd.data_ptr() and torch.equal(R.bits(gd), R.bits(gy)), what + " wrote gy"
        R.same_bits(gout, R.relu_mask_statement(gy, y), what)
        two = gy.cuda()
        ops.relu_bwd_chansum(code, two, yd, None, True)
        assert torch.equal(R.bits(gout), R.bits(two)), what + ": not the in-place route's bits"
        _sums(gb, gy, cnt, what + " sums")


@pytest.mark.parametrize("C", (12, 64))
@pytest.mark.parametrize("dtype", DTYPES)
def test_relu_family_non_finite_gradients(dtype, C, set_opt):
    """+-inf and NaN in two channels of gy, at kept and at masked positions: a masked one comes out +0.0 (a product would make it
    NaN), a kept one keeps its bits, the other channels' sums stay within their bound, the two channels' sums are non-finite."""
    ops, code, td = pkg("ops"), R.CODE[dtype], R.TDT[dtype]
    set_opt("CHANSUM_KTHREADS", 1)
    npix = _npix_list(C)[7]                                      # three trips and one pixel
    y, gy, cnt = [t.clone() for t in _relu_inputs(npix, C, dtype)]
    bad = (2, C - 1)
    rows = torch.arange(3, npix, 17)
    vals = torch.tensor([float("inf"), float("-inf"), float("nan")]).to(td)
    for ch in bad:
        gy[rows, ch] = vals[(rows + ch) % 3]
        y[rows, ch] = (rows % 2).to(td)                          # kept, masked, kept, ...
    kept = torch.zeros_like(y, dtype=torch.bool)
    masked = torch.zeros_like(y, dtype=torch.bool)
    for ch in bad:
        kept[rows[rows % 2 == 1], ch] = True
        masked[rows[rows % 2 == 0], ch] = True
    assert int(kept.sum()) >= 6 and int(masked.sum()) >= 6 and not bool(torch.isfinite(gy[kept].float()).any())
    good = torch.tensor([c not in bad for c in range(C)])
    want = R.relu_mask_statement(gy, y)
    assert int(R.bits(want)[masked].abs().sum()) == 0
    yd, cd = y.cuda(), cnt.cuda()

    def check_sums(buf, g, k, what):
        buf = buf.cpu()
        assert not bool(torch.isfinite(buf[~good]).any()), what + ": a polluted channel's sum is finite"
        w, n, A = R.chansum_statement(g.float()[:, good], k, INIT)
        R.assert_within(buf[good], w, n, A, torch.float32, what)

    gd, gsum = gy.cuda(), torch.full((C,), INIT, device="cuda")
    ops.relu_bwd_chansum(code, gd, yd, gsum, True)
    R.same_bits(gd, want, "relu_bwd_chansum non-finite")
    assert int(R.bits(gd)[masked].abs().sum()) == 0
    check_sums(gsum, want, None, "relu_bwd_chansum non-finite sums")
    gd, gb = gy.cuda(), torch.full((C,), INIT, device="cuda")
    gout = ops.relu_mask_rowscale_bwd(code, gd, yd, cd, gb)
    R.same_bits(gout, want, "relu_mask_rowscale_bwd non-finite")
    assert int(R.bits(gout)[masked].abs().sum()) == 0 and torch.equal(R.bits(gd), R.bits(gy))
    check_sums(gb, gy, cnt, "relu_mask_rowscale_bwd non-finite sums")
    gb = torch.full((C,), INIT, device="cuda")
    ops.rowscale_bias_bwd(code, gd, cd, gb)
    check_sums(gb, gy, cnt, "rowscale_bias_bwd non-finite sums")


@pytest.mark.parametrize("C", RELU_C)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rowscale_bias_fwd_edges(dtype, C):
    """y + cnt * b2 in place: two terms, stored in the tensor's type.  |y| in [1, 2) and |b2| <= 0.25: no result below 0.25 (fp16)."""
    ops, code, td = pkg("ops"), R.CODE[dtype], R.TDT[dtype]
    for npix in (1, 257, 1025):
        u = rnd((npix, C), 60 + npix % 3)
        y = (torch.where(u < 0, u - 1.0, u + 1.0)).to(td)
        b2 = rnd((C,), 61, -0.25, 0.25)
        g = torch.Generator().manual_seed(npix)
        cnt = torch.randint(0, 4, (npix,), generator=g).float()
        cnt[npix // 2:npix // 2 + npix // 4] = 0.0
        want, n, A = R.rowscale_bias_fwd_statement(y, cnt, b2)
        assert n == 2 and float(want.abs().min()) >= 0.25
        yd = y.cuda()
        out = ops.rowscale_bias_fwd(code, yd, cnt.cuda(), b2.cuda())
        assert out.data_ptr() == yd.data_ptr()
        R.assert_within(out.float(), want, n, A, td, "rowscale_bias_fwd %s C=%d npix=%d" % (dtype, C, npix))
        zero_rows = cnt == 0
        if bool(zero_rows.any()):
            assert torch.equal(R.bits(out.cpu()[zero_rows]), R.bits(y[zero_rows]))          # + 0 * b2: the value itself


# ------------------------------------------------------------------------------------------------------------------ resize
def _shape_id(s):
    return "%dx%d_to_%dx%d" % (s[0] + s[1])


def _check_matrices(in_hw, out_hw, align):
    """Every output's weights in the statement are non-negative and add up to 1 within 2^-22, in both variants."""
    for fused in (False, True):
        for W in R.resize_matrices(in_hw, out_hw, align, fused):
            assert float(W.min()) >= 0 and float((W.sum(1) - 1).abs().max()) <= 2.0 ** -22


def _resize_values(shape, seed, dtype):
    """[B,H,W,C] in the storage type: uniform in +-1; for fp16 in [0.25, 1], so that no stored result is subnormal."""
    if dtype == "f16":
        return rnd(shape, seed, 0.25, 1.0).to(torch.float16)
    return rnd(shape, seed).to(R.TDT[dtype])


@pytest.mark.parametrize("shape", R.RESIZE_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_fwd_edges(dtype, align, shape):
    ops, code, td = pkg("ops"), R.CODE[dtype], R.TDT[dtype]
    (hi, wi), (ho, wo) = shape
    _check_matrices((hi, wi), (ho, wo), align)
    for C in (4, 8, 12):
        x = _resize_values((2, hi, wi, C), 70 + C, dtype)
        add = _resize_values((2, ho, wo, C), 71 + C, dtype)
        for a in (None, add):
            what = "resize_fwd %s align=%d %s C=%d add=%d" % (dtype, align, _shape_id(shape), C, a is not None)
            y = ops.resize_bilinear_fwd(code, x.cuda(), (ho, wo), align, None if a is None else a.cuda())
            stm = [R.resize_fwd_statement(x, (ho, wo), align, fused, a) for fused in (False, True)]
            print(what, "->", R.assert_one_variant(y.float(), stm[0], stm[1], td, what))


def _bwd_gys(shape, C, dtype, align, in_hw):
    """Upstream gradients [B,Ho,Wo,C] of the storage type: uniform; for fp32 also an integer-valued one; for fp16 positive and
    scaled by the power of two, chosen from the statement, that lifts the smallest non-zero result to 2^-14."""
    if dtype == "f32":
        g = torch.Generator().manual_seed(C)
        return [rnd(shape, 80 + C), torch.randint(-3, 4, shape, generator=g).float()]
    if dtype == "bf16":
        return [rnd(shape, 80 + C).to(torch.bfloat16)]
    gy = rnd(shape, 80 + C, 0.5, 1.0).to(torch.float16)
    lo, hi = float("inf"), 0.0
    for fused in (False, True):
        want = R.resize_bwd_statement(gy, in_hw, align, fused)[0]
        lo, hi = min(lo, float(want[want > 0].min())), max(hi, float(want.max()))
    k = max(0, int(np.ceil(np.log2(2.0 ** -14 / lo))))
    assert k <= 15 and hi * 2.0 ** k <= 32768.0, "no power of two puts the fp16 results between 2^-14 and 2^15"
    return [(gy.float() * 2.0 ** k).to(torch.float16)]


@pytest.mark.parametrize("shape", R.RESIZE_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_bwd_edges(dtype, align, shape):
    ops, code, td = pkg("ops"), R.CODE[dtype], R.TDT[dtype]
    (hi, wi), (ho, wo) = shape
    _check_matrices((hi, wi), (ho, wo), align)
    for C in (4, 8, 12):
        for j, gy in enumerate(_bwd_gys((2, ho, wo, C), C, dtype, align, (hi, wi))):
            what = "resize_bwd %s align=%d %s C=%d gy#%d" % (dtype, align, _shape_id(shape), C, j)
            gd = gy.cuda()
            gx = ops.resize_bilinear_bwd(code, gd, (hi, wi), align)
            assert torch.equal(R.bits(gd), R.bits(gy)), what + " wrote gy"
            stm = [R.resize_bwd_statement(gy, (hi, wi), align, fused) for fused in (False, True)]
            print(what, "->", R.assert_one_variant(gx.float(), stm[0], stm[1], td, what))


PARENT_CASES = [(dtype, align, i) for dtype in ("f32", "bf16") for align in (0, 1) for i in (0, 1)]


def parent_case_gy(dtype, align, i):
    """The upstream gradient of one fixture entry: production's two resize shapes, B = 1, C = 8 (the 8-channel instantiation)."""
    (hi, wi), (ho, wo) = R.RESIZE_SHAPES[i]
    return rnd((1, ho, wo, 8), 90 + 2 * i + align).to(R.TDT[dtype]), (hi, wi)


@pytest.mark.parametrize("case", PARENT_CASES, ids=["%s_align%d_%d" % c for c in PARENT_CASES])
def test_resize_bwd_production_shapes_keep_their_bits(case):
    """The window fix visits the same non-zero candidates in the same order wherever the old window was complete, so at production's
    x2 shapes the input gradient is bit for bit what the library computed before the fix.  tests/golden/resize_bwd_parent.npz holds
    those bits: dcf_resize_bilinear_bwd of the commit before the fix on an MI355X, fed parent_case_gy()."""
    ops = pkg("ops")
    dtype, align, i = case
    gy, in_hw = parent_case_gy(dtype, align, i)
    gx = ops.resize_bilinear_bwd(R.CODE[dtype], gy.cuda(), in_hw, align)
    with np.load(PARENT_FIXTURE, allow_pickle=False) as z:
        want = torch.from_numpy(z["gx_%s_align%d_%d" % case])
    got = R.bits(gx)
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got, want), "%d of %d elements differ from the parent's bits" % (int((got != want).sum()), got.numel())
