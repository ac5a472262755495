"""The statements of tests/_elementwise_ref.py against ATen in fp64 and against their own contracts, and the candidate window of
k_resize_bwd restated -- so that a wrong statement cannot bless a wrong kernel (tests/test_gpu_elementwise_edges.py).  CPU only.

The resize statement and F.interpolate in fp64 differ only through the fp32 rounding of the source coordinate.  Measured over
R.RESIZE_SHAPES on the CPU (both tests print their figures): a weight differs from the exact coordinate's by at most 1.3e-6 under
align_corners = 0 and 4.2e-6 under align_corners = 1 (coordinates up to 155); against ATen the largest |diff| / A is 2.8e-6 / 1.0e-5
in the forward and 1.1e-5 / 1.5e-5 in the backward, the inputs having magnitudes in [0.5, 1.5).  A wrong tap or clamp errs by at
least 1 / (2 * ratio) of a tap, 0.03 at the largest factor here.  RESIZE_RTOL = 1e-4 of A, element by element, is six times the
largest figure measured and 300 times below the smallest wrong tap."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as CR
import _elementwise_ref as R

RESIZE_RTOL = 1e-4              # measured against ATen fp64 on the CPU: 1.5e-5 of A at the most (see the module docstring)
DTYPES = ["f32", "bf16", "f16"]


# ---------------------------------------------------------------------------------------------------------------- resize
def _signed(shape, g):
    """Magnitudes in [0.5, 1.5) with random signs: |diff| / A then measures the weights -- with values near zero a term's share of A
    can be arbitrarily small and the ratio says nothing about them."""
    mag = torch.rand(shape, generator=g, dtype=torch.float64) + 0.5
    return torch.where(torch.rand(shape, generator=g) < 0.5, -mag, mag)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("align", [0, 1])
def test_resize_statement_against_interpolate(align, fused):
    """Forward and backward of every shape against F.interpolate and its autograd in fp64, |diff| <= 1e-4 * A element by element."""
    g = torch.Generator().manual_seed(11)
    worst_f = worst_b = 0.0
    for (hi, wi), (ho, wo) in R.RESIZE_SHAPES:
        x, gy = _signed((2, hi, wi, 4), g), _signed((2, ho, wo, 4), g)
        add = (torch.rand(2, ho, wo, 4, generator=g, dtype=torch.float64) - 0.5)
        xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        ref = F.interpolate(xn, size=(ho, wo), mode="bilinear", align_corners=bool(align))
        ref.backward(gy.permute(0, 3, 1, 2))
        want, n, A = R.resize_fwd_statement(x, (ho, wo), align, fused, add)
        d = (want - (ref.detach().permute(0, 2, 3, 1) + add)).abs()
        assert n == 5 and bool((d <= RESIZE_RTOL * A).all()), ((hi, wi), (ho, wo), float((d / A).max()))
        worst_f = max(worst_f, float((d / A.clamp(min=1e-300)).max()))
        gwant, gn, gA = R.resize_bwd_statement(gy, (hi, wi), align, fused)
        gd = (gwant - xn.grad.permute(0, 2, 3, 1)).abs()
        assert bool((gd <= RESIZE_RTOL * gA).all()), ((hi, wi), (ho, wo), float((gd / gA.clamp(min=1e-300)).max()))
        assert bool(((gA != 0) | (xn.grad.permute(0, 2, 3, 1) == 0)).all())            # no contribution: exactly zero on both sides
        worst_b = max(worst_b, float((gd / gA.clamp(min=1e-300)).max()))
    print("align %d fused %d: largest |diff| / A forward %.3g, backward %.3g" % (align, fused, worst_f, worst_b))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("align", [0, 1])
def test_resize_matrices_are_interpolations(align, fused):
    """Every output's weights are non-negative and add up to 1 within 2^-22 (1 - l is rounded once in fp32), at most two of them
    are non-zero, and they sit on adjacent inputs; the backward's n counts the outputs that sample one input."""
    worst = 0.0
    for (hi, wi), (ho, wo) in R.RESIZE_SHAPES:
        for n_in, n_out in ((hi, ho), (wi, wo)):
            W = R.resize_matrix(n_in, n_out, align, fused)
            assert tuple(W.shape) == (n_out, n_in) and float(W.min()) >= 0
            assert float((W.sum(1) - 1).abs().max()) <= 2.0 ** -22
            i0, i1, l = R.src_index(n_in, n_out, align, fused)
            assert bool(((i1 - i0 >= 0) & (i1 - i0 <= 1) & (i0 >= 0) & (i1 <= n_in - 1)).all()) and float(l.min()) >= 0 and float(l.max()) <= 1
            assert int((W != 0).sum(1).max()) <= 2
            # against the exact coordinate: the fp32 one is off by a few ulp of the coordinate, far below one tap
            o = np.arange(n_out, dtype=np.float64)
            if align:
                s = o * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
            else:
                s = np.maximum((o + 0.5) * (n_in / n_out) - 0.5, 0.0)
            s = np.minimum(s, n_in - 1)
            Wx = np.zeros((n_out, n_in))
            f = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
            c = np.minimum(f + 1, n_in - 1)
            np.add.at(Wx, (np.arange(n_out), f), 1 - (s - f))
            np.add.at(Wx, (np.arange(n_out), c), s - f)
            worst = max(worst, float(np.abs(W.numpy() - Wx).max()))
    print("align %d fused %d: largest weight difference to the exact coordinate %.3g" % (align, fused, worst))
    assert worst <= 1e-5


def test_fused_and_unfused_differ_somewhere():
    """The flag is not idle: on some shape of the list the two roundings of the source coordinate give another weight (and under
    align_corners = 1, where there is no multiply-add to contract, never)."""
    differ = 0
    for (hi, wi), (ho, wo) in R.RESIZE_SHAPES:
        for n_in, n_out in ((hi, ho), (wi, wo)):
            differ += int(not torch.equal(R.resize_matrix(n_in, n_out, 0, False), R.resize_matrix(n_in, n_out, 0, True)))
            assert torch.equal(R.resize_matrix(n_in, n_out, 1, False), R.resize_matrix(n_in, n_out, 1, True))
    assert differ > 0


def _outside(n_in, n_out, align, fixed):
    """(input, output) pairs with a non-zero weight in either statement variant that the backward's window does not visit."""
    lo, hi = R.resize_bwd_window(n_in, n_out, align, fixed)
    out = []
    for fused in (False, True):
        W = R.resize_matrix(n_in, n_out, align, fused).numpy()
        o, i = np.nonzero(W)
        miss = (o < lo[i]) | (o > hi[i])
        out += [(int(a), int(b), float(W[b, a])) for a, b in zip(i[miss], o[miss])]
    return out


@pytest.mark.parametrize("align", [0, 1])
def test_resize_bwd_window_covers_every_weight(align):
    """No (input, output) pair with a non-zero weight lies outside the window k_resize_bwd searches, on either axis of any shape."""
    for (hi, wi), (ho, wo) in R.RESIZE_SHAPES:
        for n_in, n_out in ((hi, ho), (wi, wo)):
            assert _outside(n_in, n_out, align, True) == [], (n_in, n_out)
    for n_in in range(1, 12):                                    # and beyond the list: every pair of sizes up to a factor of 24
        for n_out in range(1, 49):
            assert _outside(n_in, n_out, align, True) == [], (n_in, n_out)


def test_resize_bwd_old_window_loses_weight_at_x8():
    """The window before the fix: complete at every factor below 8 and under align_corners = 1, short of a tap of weight 1/16 at
    4 -> 32 and 22 -> 176 and of more beyond."""
    lost = {k: max([w for _, _, w in _outside(k[0], k[1], 0, False)] or [0.0]) for k in ((4, 32), (22, 176), (2, 33), (3, 48))}
    print("weight lost per pair by the old window:", lost)
    assert lost[(4, 32)] == 0.0625 and lost[(22, 176)] == 0.0625 and lost[(2, 33)] > 0.25 and lost[(3, 48)] > 0.28
    for (hi, wi), (ho, wo) in R.RESIZE_SHAPES:
        for n_in, n_out in ((hi, ho), (wi, wo)):
            assert _outside(n_in, n_out, 1, False) == []
            if n_out < 8 * n_in:
                assert _outside(n_in, n_out, 0, False) == [], (n_in, n_out)
    for (hi, wi), (ho, wo) in R.LARGE_FACTOR_SHAPES:
        assert _outside(hi, ho, 0, False) or _outside(wi, wo, 0, False), ((hi, wi), (ho, wo))


def test_resize_window_fix_keeps_the_visit_order():
    """Both windows are contiguous ranges walked in ascending order and zero weights are skipped: wherever the old window was
    complete the two visit the same non-zero candidates in the same order, so those sums are bit for bit the same.  Under
    align_corners = 1 and at an exact x2 the window itself is unchanged, and at production's shapes it is never longer."""
    for k, ((hi, wi), (ho, wo)) in enumerate(R.RESIZE_SHAPES):
        for n_in, n_out in ((hi, ho), (wi, wo)):
            for align in (0, 1):
                lo0, hi0 = R.resize_bwd_window(n_in, n_out, align, False)
                lo1, hi1 = R.resize_bwd_window(n_in, n_out, align, True)
                assert np.array_equal(lo0, lo1)
                if align or n_out == 2 * n_in:
                    assert np.array_equal(hi0, hi1), (n_in, n_out, align)
                if k < 2:                                        # production's shapes, x2 and 24 -> 47: never a longer search
                    assert bool((hi1 <= hi0).all()), (n_in, n_out, align)
                if _outside(n_in, n_out, align, False):
                    continue
                for fused in (False, True):
                    W = R.resize_matrix(n_in, n_out, align, fused).numpy()
                    for i in range(n_in):
                        old = [o for o in range(lo0[i], hi0[i] + 1) if W[o, i] != 0]
                        new = [o for o in range(lo1[i], hi1[i] + 1) if W[o, i] != 0]
                        assert old == new, (n_in, n_out, align, i)


# ---------------------------------------------------------------------------------------------------------------- ReLU family
@pytest.mark.parametrize("dtype", DTYPES)
def test_relu_mask_statement_against_threshold_backward(dtype):
    """The select against ATen's threshold backward, bit for bit, on a y with -0.0, subnormals and exact zeros and a gy with
    infinities and NaN at kept and at masked positions."""
    td = R.TDT[dtype]
    g = torch.Generator().manual_seed(5)
    y = torch.relu(torch.rand(64, 8, generator=g) - 0.6).to(td)
    y[0, :4] = torch.tensor([-0.0, R.SMALLEST_SUBNORMAL[td], -R.SMALLEST_SUBNORMAL[td], 0.0], dtype=torch.float64).to(td)
    gy = (torch.rand(64, 8, generator=g) - 0.5).to(td)
    gy[1] = torch.tensor([float("inf"), float("-inf"), float("nan"), -1.0] * 2).to(td)
    gy[2] = gy[1]
    y[1], y[2] = 1.0, 0.0
    want = R.relu_mask_statement(gy, y)
    R.same_bits(want, torch.ops.aten.threshold_backward(gy, y, 0), dtype)
    assert int(R.bits(want[2]).abs().sum()) == 0                               # masked: +0.0 bits, whatever gy held
    assert int(R.bits(want[0, 0])) == 0 and int(R.bits(want[0, 2])) == 0 and int(R.bits(want[0, 3])) == 0
    assert int(R.bits(want[0, 1])) == int(R.bits(gy[0, 1]))                    # the smallest subnormal is > 0: kept


def test_chansum_statement():
    g = torch.Generator().manual_seed(6)
    gy = torch.rand(37, 12, generator=g) - 0.5
    cnt = torch.randint(0, 4, (37,), generator=g).float()
    want, n, A = R.chansum_statement(gy, cnt, 0.25)
    lit = torch.stack([sum(float(cnt[p]) * float(gy[p, c]) for p in range(37)) + torch.tensor(0.25, dtype=torch.float64) for c in range(12)])
    assert n == 38 and float((want - lit).abs().max()) <= 1e-13
    assert float((A - ((cnt[:, None].double() * gy.double()).abs().sum(0) + 0.25)).abs().max()) <= 1e-13
    w1, n1, A1 = R.chansum_statement(gy, None, 0.0)
    assert n1 == 38 and float((w1 - gy.double().sum(0)).abs().max()) <= 1e-13 and float((A1 - gy.double().abs().sum(0)).abs().max()) <= 1e-13
    y, b2 = torch.rand(37, 12, generator=g), torch.rand(12, generator=g) - 0.5
    fw, fn, fA = R.rowscale_bias_fwd_statement(y, cnt, b2)
    assert fn == 2 and torch.equal(fw, y.double() + cnt.double()[:, None] * b2.double()[None]) and bool((fA >= fw.abs()).all())


def test_chan_stride_reaches_every_loop():
    """With CHANSUM_KTHREADS = 1 the walk has 1023 threads for three channel groups and 1024 otherwise."""
    for C, cg, stride in ((4, 1, 1024), (8, 1, 1024), (12, 3, 1023), (24, 3, 1023), (64, 8, 1024)):
        V, g, nvec, s = R.chan_stride(10 ** 6, C, 1)
        assert (g, s) == (cg, stride) and V * g == C and nvec == 10 ** 6 * cg
        assert R.chan_stride(5, C, 1)[3] == 5 * cg                                 # a tensor smaller than the grid: one trip


# ---------------------------------------------------------------------------------------------------------------- layout and cast
@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_and_cast_statements(dtype):
    td = R.TDT[dtype]
    x = R.table_tensor((2, 12, 3, 5), 3)
    y = R.nchw_to_nhwc_statement(x, td)
    assert y.dtype == td and tuple(y.shape) == (2, 3, 5, 12)
    for b in range(2):
        for c in range(12):
            R.same_bits(y[b, :, :, c], x[b, c].to(td), "nchw_to_nhwc")
    back = R.nhwc_to_nchw_statement(y)
    assert back.dtype == torch.float32
    R.same_bits(back, x.to(td).float(), "nhwc_to_nchw")
    R.same_bits(R.cast_statement(x, td), x.to(td), "cast")
    if dtype == "f32":
        R.same_bits(back, x, "round trip")


def test_value_table_census_and_roundings():
    """The table holds every class it names, and torch's CPU conversion -- the statement -- rounds them to nearest even."""
    t = R.value_table()
    c = R.table_census(t)
    assert all(v >= 1 for v in c.values()), c
    assert c["+0"] == 1 and c["-0"] == 1 and c["nan"] == 1 and c["f16_subnormal"] == 2
    c2 = R.table_census(R.table_tensor((2, 36, 17, 16), 4))
    assert all(c2[k] >= c[k] for k in c), c2
    h = lambda v: float(torch.tensor(v, dtype=torch.float32).to(torch.float16))
    b = lambda v: float(torch.tensor(v, dtype=torch.float32).to(torch.bfloat16))
    assert h(65519.0) == 65504.0 and h(65520.0) == float("inf") and h(65536.0) == float("inf") and h(-65520.0) == float("-inf")
    assert h(2.0 ** -25) == 0.0 and h(3 * 2.0 ** -25) == 2.0 ** -23 and h(2.0 ** -24) == 2.0 ** -24
    assert h(1 + 2.0 ** -11) == 1.0 and h(1 + 2.0 ** -10 + 2.0 ** -11) == 1 + 2.0 ** -9
    assert b(1 + 2.0 ** -8) == 1.0 and b(1 + 2.0 ** -7 + 2.0 ** -8) == 1 + 2.0 ** -6
    assert b(2.0 ** -133) == 2.0 ** -133 and b(2.0 ** -134) == 0.0 and b(3 * 2.0 ** -134) == 2.0 ** -132 and b(2.0 ** -149) == 0.0
    assert b(3.4028234663852886e38) == float("inf") and b(3.3895313892515355e38) == 3.3895313892515355e38
    assert int(R.bits(torch.tensor(-0.0).to(torch.bfloat16))) == -32768 and int(R.bits(torch.tensor(-(2.0 ** -25)).to(torch.float16))) == -32768


def test_same_bits_tells_zeros_apart_and_nans_not():
    a = torch.tensor([0.0, float("nan"), 1.0])
    R.same_bits(a, torch.tensor([0.0, float("nan"), 1.0]), "same")
    R.same_bits(a, torch.from_numpy(np.array([0, 0x7fc01234, 0x3f800000], dtype=np.uint32).view(np.float32).copy()), "payload")
    with pytest.raises(AssertionError):
        R.same_bits(a, torch.tensor([-0.0, float("nan"), 1.0]), "zero")
    with pytest.raises(AssertionError):
        R.same_bits(a, torch.tensor([0.0, 1.0, 1.0]), "nan")


@pytest.mark.parametrize("dtype", DTYPES)
def test_image_statement_against_conv_ref(dtype):
    """Against the fp64 construction the convolution tests use (tests/_conv_ref.py::image_nhwc4): the interior agrees to one fp32
    rounding (and the store's), everything outside it is +0.0 bit for bit."""
    td = R.TDT[dtype]
    for (H, W) in ((1, 1), (5, 3), (16, 8)):
        g = torch.Generator().manual_seed(H)
        img = torch.randint(0, 256, (2, 3, H, W), generator=g, dtype=torch.int64).to(torch.uint8)
        img.view(-1)[:min(256, img.numel())] = torch.arange(min(256, img.numel())).to(torch.uint8)
        want = R.image_statement(img, td)
        ref = CR.image_nhwc4(img)
        assert tuple(want.shape) == tuple(ref.shape) == (2, H + 6, W + 8, 4)
        inside = R.image_interior_mask(2, H, W)
        assert int(R.bits(want)[~inside].abs().sum()) == 0 and float(ref[~inside].abs().max()) == 0.0
        err = (want.double() - ref).abs()
        assert bool((err <= (2.0 ** -24 + R.STORE_ULP[td]) * ref.abs()).all()), float(err.max())
        if td == torch.float32:
            assert torch.equal(want, ref.float())                # the correctly rounded quotient IS the rounded fp64 quotient here
