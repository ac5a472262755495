"""The fp8 statements of tests/_fp8_ref.py on the CPU: the integer e4m3 codec against torch's float8_e4m3fn conversion (two
independent statements that must agree), the properties of the exact scale rule, and -- on the references alone -- the conditions
under which the cases of tests/test_gpu_fp8_exact.py test anything: exact accumulators and epilogue terms, and stores that round."""
import math
from fractions import Fraction

import pytest
import torch

import _conv_ref as R
import _fp8_ref as F8
import test_gpu_fp8_exact as X


# ---------------------------------------------------------------------------------------------------------------- codec
def test_decode_is_the_e4m3_grid():
    vals = [F8.decode_fraction(b) for b in range(0x7F)]
    assert vals[0] == 0 and vals[1] == Fraction(1, 512) and vals[7] == Fraction(7, 512) and vals[8] == Fraction(1, 64)
    assert vals[0x38] == 1 and vals[0x7E] == 448 and all(a < b for a, b in zip(vals, vals[1:]))
    assert F8.decode_fraction(0x7F) is None and F8.decode_fraction(0xFF) is None and math.isnan(F8.decode(0x7F))
    assert all(F8.decode_fraction(b | 0x80) == -F8.decode_fraction(b) for b in range(0x7F))
    assert math.copysign(1.0, F8.decode(0x80)) == -1.0 and F8.decode(0x80) == 0.0


def test_decode_equals_torch_on_all_256_codes():
    b = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    t = b.view(torch.float8_e4m3fn).float()
    mine = torch.tensor([F8.decode(i) for i in range(256)], dtype=torch.float32)
    assert torch.equal(torch.isnan(t), torch.isnan(mine)) and int(torch.isnan(t).sum()) == 2
    ok = ~torch.isnan(t)
    assert torch.equal(t[ok].view(torch.int32), mine[ok].view(torch.int32))          # the sign of -0 included
    assert torch.equal(F8.decode_tensor(b)[ok], mine[ok].double())


def test_encode_equals_torch_on_codes_midpoints_and_neighbours():
    vals = F8.codec_probe_values()
    assert len(vals) > 2 * (127 + 3 * 126)
    x = torch.tensor(vals, dtype=torch.float64)
    finite = ~torch.isnan(x)
    assert torch.equal(x.float().double()[finite], x[finite]), "a probe value is not an fp32 number"
    mine = torch.tensor([F8.encode(v) for v in vals], dtype=torch.uint8)
    tq = x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(mine[finite], tq[finite]), [(vals[i], int(mine[i]), int(tq[i])) for i in (mine != tq).nonzero().flatten().tolist()[:8]]
    assert int(mine[-1]) == F8.NAN_CODE and (int(tq[-1]) & 0x7F) == 0x7F
    assert torch.equal(F8.encode_tensor(x), mine)              # the table form is the same function
    # every code is a fixed point; ties go to the even code; the subnormal boundary and the saturation edge
    assert all(F8.encode(F8.decode(b)) == b for b in range(256) if b & 0x7F != 0x7F)
    for j, m in enumerate(F8.MIDPOINTS):
        assert F8.encode(float(m)) == j + (j & 1) and F8.encode(F8.f32_next(float(m), -1)) == j and F8.encode(F8.f32_next(float(m), 1)) == j + 1
    assert F8.encode(2.0 ** -10) == 0 and F8.encode(-2.0 ** -10) == 0x80 and F8.encode(3 * 2.0 ** -10) == 2
    assert F8.encode(7.5 * 2.0 ** -9) == 8 and F8.encode(-0.0) == 0x80 and F8.encode(0.0) == 0
    assert [F8.encode(v) for v in (448.0, 464.0, 465.0, 1e30, float("inf"), -464.0, float("-inf"))] == [0x7E] * 5 + [0xFE] * 2
    assert F8.encode(float("nan")) == F8.NAN_CODE


# ---------------------------------------------------------------------------------------------------------------- scale rule
def test_scale_rule_properties():
    vals = F8.scale_rule_values()
    assert len(vals) > 7 * 270
    for a in vals:
        s = F8.act_scale_exact(a)
        if not (a == a and 0.0 < a < float("inf")):
            assert s == 1.0
            continue
        m, e = math.frexp(s)
        assert m == 0.5 and e - 1 <= 126                       # a power of two, at most 2^126
        assert Fraction(a) * Fraction(s) <= 224
        assert e - 1 == 126 or Fraction(a) * Fraction(s) * 2 > 224
        assert F8.f32(1.0 / s) == 1.0 / s and 1.0 / s >= F8.FLT_MIN                  # 1 / s is a normal fp32 number
    S = F8.act_scale_exact
    assert S(224.0) == 1.0 and S(F8.f32_next(224.0, 1)) == 0.5 and S(F8.f32_next(224.0, -1)) == 1.0 and S(100.0) == 2.0
    assert S(F8.FLT_TRUE_MIN) == S(1e-40) == S(F8.FLT_MIN) == S(6.5e-37) == 2.0 ** 126
    assert S(6.6e-37) == 2.0 ** 126 and S(1.4e-36) == 2.0 ** 126 and S(2.6e-36) == 2.0 ** 126 and S(2.7e-36) == 2.0 ** 125
    assert S(3.0e38) == S(F8.FLT_MAX) == 2.0 ** -121 and S(2.9e38) == S(F8.f32(math.ldexp(224.0, 120))) == 2.0 ** -120
    assert S(float("inf")) == S(float("nan")) == S(0.0) == S(-3.0) == 1.0


# ---------------------------------------------------------------------------------------------------------------- conv references
def _unique(key):
    seen, out = set(), []
    for c in X.CONV_CASES:
        k = key(c)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


def test_case_table_is_sound():
    ids = [X.case_id(c) for c in X.CONV_CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in set(ids) if ids.count(i) > 1)
    forced = {}
    for c in X.CONV_CASES:
        B, H, W, Cin, Cout, kh, kw, s, p = c.shape
        bn, bm = X.TILE_DIMS[c.frag]
        assert Cin % 64 == 0 and Cout % bn == 0 and c.maker in F8.MAKERS
        M = B * R.out_size(H, kh, s, p) * R.out_size(W, kw, s, p)
        blocks = lambda n, m: -(-M // m) * (Cout // n)
        opts = dict(c.opts)
        if "F8_TILE" in opts:
            forced.setdefault(c.frag, set()).add(blocks(bn, bm))
            want = {0: X.T0, 1: X.T1, 2: X.T2, 3: X.FA if Cout % 64 == 0 else X.FB}[opts["F8_TILE"]]
        elif blocks(128, 128) >= 512 and Cout % 128 == 0:
            want = X.T0
        elif blocks(64, 256) >= 512 and Cout % 64 == 0:
            want = X.T1
        elif blocks(64, 128) >= 256 and Cout % 64 == 0:
            want = X.T2
        else:
            want = X.FA if Cout % 64 == 0 else X.FB
        assert c.frag == want, X.case_id(c)
    # every instantiation is forced, on fewer than 8 tiles, exactly 8, and more than 8 that are no multiple of 8
    assert set(forced) == set(X.TILE_DIMS)
    for frag, counts in forced.items():
        assert any(n < 8 for n in counts) and 8 in counts and any(n > 8 and n % 8 for n in counts), (frag, sorted(counts))
    # and launch_f8's own thresholds reach each of the three large tiles
    assert {c.frag for c in X.CONV_CASES if "F8_TILE" not in dict(c.opts)} == {X.T0, X.T1, X.T2, X.FA}


@pytest.mark.parametrize("case", _unique(lambda c: (c.shape, c.maker)), ids=X.case_id)
def test_accumulators_and_epilogue_terms_are_exact(case):
    """operands() asserts the accumulator bound, conv_reference() that the product and both sums are fp32 values; here: the images
    decode to the operands, the plain result is the convolution of the decoded images, and both y8 maxima do what they are for."""
    ref, plain, fused = F8.conv_reference(case.shape, R.F32, case.maker)
    B, H, W, Cin, Cout, kh, kw, s, p = case.shape
    x = F8.decode_tensor(ref["x8"]) / ref["sx"]
    w = F8.decode_tensor(ref["w8"]) * ref["wscale"].view(-1, 1, 1, 1)
    if B * H * W <= 4096:
        want = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), None, s, p).permute(0, 2, 3, 1)
        assert torch.equal(plain, want)
    factors = set((ref["wscale"] / (512.0 if case.maker == "subnormal" else 1.0)).tolist())
    assert factors <= {0.5, 1.0, 2.0, 4.0} and len(factors) >= 3
    assert bool((fused >= 0).all()) and float(plain.abs().max()) > 0
    for dt in X.DTYPES:
        _, sy1, m1 = F8.expect_y8(plain, dt, F8.y8_amax(plain, dt, False))
        img2, sy2, m2 = F8.expect_y8(fused, dt, F8.y8_amax(fused, dt, True))
        assert m1 * sy1 <= 224.0 and m2 * sy2 > 448.0
        sat = float((img2 == 0x7E).sum()) / img2.numel()
        assert 0.0 < sat < 0.5, "%.1f%% of the fused image saturates" % (100 * sat)


@pytest.mark.parametrize("dt", [R.BF16, R.F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", _unique(lambda c: (c.shape, c.maker)), ids=X.case_id)
def test_fused_cases_make_the_store_round(case, dt):
    """>= 8% of the outputs not representable in the storage type, >= 4% exact ties, 30-70% alive after the ReLU."""
    R.assert_census(F8.conv_reference(case.shape, dt, case.maker)[2], dt, X.case_id(case))
