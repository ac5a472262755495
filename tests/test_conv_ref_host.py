"""The fp64 convolution statements of tests/_conv_ref.py against torch's fp64 convolution and its autograd (exact equality on
the integer inputs), the exact-bit helper on hand-written ties, and -- on the references alone -- the conditions under which
the fused 16-bit cases of tests/test_gpu_conv_exact.py exercise the rounding of the store at all."""
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
import test_gpu_conv_exact as X

# (B, H, W, Cin, Cout, kh, kw, stride, pad): non-square kernels, 5x5 / 7x7, pads 0..3, stride 2 on odd sizes
STATEMENT_SHAPES = [
    (2, 9, 11, 8, 6, 1, 3, 1, 0), (2, 9, 11, 8, 6, 1, 3, 1, 1), (1, 11, 9, 5, 7, 3, 1, 1, 0), (1, 11, 9, 5, 7, 3, 1, 2, 1),
    (2, 11, 13, 4, 8, 5, 5, 1, 2), (1, 13, 11, 4, 8, 5, 5, 2, 2), (1, 13, 11, 4, 8, 5, 5, 2, 0), (1, 9, 10, 3, 5, 7, 7, 1, 3),
    (2, 15, 13, 3, 5, 7, 7, 2, 3), (2, 15, 13, 3, 5, 7, 7, 2, 1), (2, 9, 11, 8, 8, 3, 3, 1, 0), (2, 9, 11, 8, 8, 3, 3, 1, 1),
    (2, 9, 11, 8, 8, 3, 3, 1, 2), (2, 9, 11, 8, 8, 3, 3, 1, 3), (2, 17, 13, 8, 8, 3, 3, 2, 1), (2, 10, 9, 8, 8, 3, 3, 2, 0),
    (2, 15, 11, 8, 12, 1, 1, 2, 0), (1, 8, 8, 16, 8, 1, 1, 1, 0), (1, 9, 79, 4, 4, 3, 3, 2, 1),
]


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("shape", STATEMENT_SHAPES)
def test_statements_equal_torch_fp64(shape):
    B, H, W, Cin, Cout, kh, kw, s, p = shape
    d = R.make_fwd(shape, R.BF16)
    x = _nchw(d["x"]).requires_grad_(True)
    w = d["w"].permute(0, 3, 1, 2).contiguous().requires_grad_(True)          # [Cout,Cin,kh,kw]
    y = F.conv2d(x, w, None, s, p)
    assert torch.equal(R.conv_lin(d["x"], d["w"], s, p), y.detach().permute(0, 2, 3, 1))
    fused = torch.relu(y.detach() + d["shift"].view(1, -1, 1, 1) + _nchw(d["res"]))
    assert torch.equal(R.conv_fwd(d["x"], d["w"], s, p, d["shift"], None, d["res"], True), fused.permute(0, 2, 3, 1))
    rs = d["rowscale"].view(B, 1, y.shape[2], y.shape[3])
    assert torch.equal(R.conv_fwd(d["x"], d["w"], s, p, d["shift"], d["rowscale"], d["res"], False),
                       (y.detach() + rs * d["shift"].view(1, -1, 1, 1) + _nchw(d["res"])).permute(0, 2, 3, 1))
    g = R.make_dgrad(shape, R.BF16)
    y.backward(_nchw(g["gy"]))
    wt = w.detach().permute(1, 2, 3, 0).contiguous()                           # [Cin,kh,kw,Cout]
    gx = x.grad.permute(0, 2, 3, 1)
    assert torch.equal(R.dgrad_lin(g["gy"], wt, (H, W), s, p), gx)
    full = torch.zeros_like(gx)
    full[:, ::2, ::2] = g["resq"]
    want = (gx + g["res"] + full) * (g["mask"] > 0)
    assert torch.equal(R.conv_dgrad(g["gy"], wt, (H, W), s, p, g["res"], g["resq"], g["mask"]), want)
    assert bool((g["mask"] > 0).any()) and bool((g["mask"] == 0).any()) and bool((g["mask"] < 0).any())
    G, gs = R.conv_wgrad(d["x"], g["gy"], kh, kw, s, p)
    assert torch.equal(G, w.grad.permute(0, 2, 3, 1)) and torch.equal(gs, g["gy"].sum((0, 1, 2)))


def test_stem_statement_equals_torch_fp64():
    shape = (2, 22, 30, 32)
    d, lin, fused, G, gs = R.stem_reference(shape, R.BF16)
    x = (d["img"].double() / 255.0).requires_grad_(False)
    assert set(torch.unique(x).tolist()) == {0.0, 1.0}
    w = d["w"].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(x, w, None, 2, 3)
    assert torch.equal(lin, y.detach().permute(0, 2, 3, 1))
    y.backward(_nchw(d["gy"]))
    assert torch.equal(G[:, :, :7, :3], w.grad.permute(0, 2, 3, 1))
    assert float(G[:, :, :, 3].abs().max()) == 0.0                  # the padded fourth channel
    assert torch.equal(gs, d["gy"].sum((0, 1, 2)))


def _bits(v, dtype):
    return int(R.expect_bits(torch.tensor([v], dtype=torch.float64), dtype)[0]) & 0xFFFF


def _val(bits, dtype):
    return float(torch.tensor([bits], dtype=torch.int32).to(torch.int16).view(R.TORCH_DT[dtype])[0])


def test_expect_bits_rounds_ties_to_even():
    # bf16: 8 significant bits, ulp 2 in [256, 512): 257 and 259 are exact ties
    assert _val(_bits(257.0, R.BF16), R.BF16) == 256.0 and _val(_bits(259.0, R.BF16), R.BF16) == 260.0
    assert _val(_bits(-257.0, R.BF16), R.BF16) == -256.0 and _val(_bits(-259.0, R.BF16), R.BF16) == -260.0
    assert _bits(257.0, R.BF16) == 0x4380 and _bits(259.0, R.BF16) == 0x4382 and _bits(-257.0, R.BF16) == 0xC380
    # fp16: 11 significant bits, ulp 2 in [2048, 4096)
    assert _val(_bits(2049.0, R.F16), R.F16) == 2048.0 and _val(_bits(2051.0, R.F16), R.F16) == 2052.0
    assert _val(_bits(-2049.0, R.F16), R.F16) == -2048.0 and _val(_bits(-2051.0, R.F16), R.F16) == -2052.0
    assert _bits(2049.0, R.F16) == 0x6800 and _bits(2051.0, R.F16) == 0x6802 and _bits(-2051.0, R.F16) == 0xE802
    # not ties: above / below the half way point, and half-integer ties in the binade below
    assert _val(_bits(257.5, R.BF16), R.BF16) == 258.0 and _val(_bits(256.5, R.BF16), R.BF16) == 256.0
    assert _val(_bits(128.5, R.BF16), R.BF16) == 128.0 and _val(_bits(129.5, R.BF16), R.BF16) == 130.0
    assert _val(_bits(-1024.5, R.F16), R.F16) == -1024.0 and _val(_bits(-1025.5, R.F16), R.F16) == -1026.0
    # zeros are +0; fp32 is the identity; a value that is no fp32 number is refused
    assert _bits(-0.0, R.BF16) == 0 and _bits(0.0, R.F16) == 0
    assert int(R.expect_bits(torch.tensor([-1.5], dtype=torch.float64), R.F32)[0]) == int(torch.tensor([-1.5]).view(torch.int32)[0])
    with pytest.raises(AssertionError):
        R.expect_bits(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), R.BF16)


def test_census_counts_inexact_values_and_ties():
    v = torch.tensor([0.0, 1.0, 255.0, 256.0, 257.0, 258.0, 259.0, 257.5, 128.5, -259.0, 0.5, -300.0], dtype=torch.float64)
    inexact, ties, alive = R.census(v, R.BF16)
    assert (round(inexact * 12), round(ties * 12), round(alive * 12)) == (5, 4, 11)
    v = torch.tensor([2048.0, 2049.0, 2050.0, 2049.5, 1024.5, 1023.5, -2051.0, 0.0], dtype=torch.float64)
    inexact, ties, alive = R.census(v, R.F16)
    assert (round(inexact * 8), round(ties * 8), round(alive * 8)) == (4, 3, 7)


def _fused_16bit():
    seen, out = set(), []
    for c in X.CONV_CASES + X.STEM_CASES:
        key = (c.kind, c.shape, c.dtype)
        if c.dtype == R.F32 or not c.fused or c.kind == "stem_wgrad" or key in seen:
            continue
        seen.add(key)
        out.append(c)
    return out


@pytest.mark.parametrize("case", _fused_16bit(), ids=lambda c: "%s-%s-%s" % (c.kind, "x".join(str(v) for v in c.shape), X.DTN[c.dtype]))
def test_fused_cases_make_the_store_round(case):
    """>= 8% of the outputs not representable in the storage type, >= 4% exact ties, 30-70% alive after the ReLU / mask."""
    if case.kind in ("fwd", "rowscale"):
        exact = R.fwd_reference(case.shape, case.dtype, case.kind == "rowscale")[2]
    elif case.kind in ("dgrad", "halfres"):
        exact = R.dgrad_reference(case.shape, case.dtype, case.kind == "halfres")[2]
    else:
        exact = R.stem_reference(case.shape, case.dtype)[2]
    R.assert_census(exact, case.dtype, X.case_id(case))


def test_every_case_states_its_launch_and_ids_are_unique():
    cases = X.CONV_CASES + X.STEM_CASES + X.WGRAD_CASES
    ids = [X.case_id(c) for c in cases]
    assert len(set(ids)) == len(ids), sorted(i for i in set(ids) if ids.count(i) > 1)
    assert all(c.frag for c in cases)
    # every 16-bit forward / input-gradient case runs the fused form, except the 1x1 / stride-2 input gradient (see the table)
    plain_only = [c for c in X.CONV_CASES if not c.fused]
    assert all(c.kind == "dgrad" and c.shape[5:8] == (1, 1, 2) and c.dtype != R.F32 for c in plain_only)
