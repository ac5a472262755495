"""The fp8 (e4m3) forward path of csrc/conv_fp8.hip against exact statements (tests/_fp8_ref.py), bit for bit.

Convolution: the e4m3 images hold small exact values and every scale is a power of two, so the fp32 accumulator, the epilogue
product and its sums are exact and the store is the one rounding: y must equal RNE_storage(exact) in every bit, and the fused second
output y8 must equal encode(stored(y) * sy) in every byte.  Every case names the tile instantiation the launch must report
(conv_fwd_fp8<64,TN,TM,WN,WM>) -- forced through F8_TILE or reached by launch_f8's own thresholds.  Outputs live in guarded buffers.
Cast: dcf_cast_fp8 against the integer codec on every bf16 and fp16 bit pattern, on every e4m3 value / midpoint / midpoint
neighbour in fp32, and on a tensor large enough for several grid-stride trips and all 64 maximum slots.  Scale rule: host entry and
device-derived value against act_scale_exact.  No tolerances.

tests/test_fp8_ref_host.py reads CONV_CASES and asserts on the references alone that the fused 16-bit cases make the store round.
"""
import collections

import pytest
import torch

import _conv_ref as R
import _fp8_ref as F8
from _util import pkg
from test_gpu_conv_exact import _assert_bits, _assert_launches, _options

pytestmark = pytest.mark.gpu

F32, BF16, F16 = R.F32, R.BF16, R.F16
DTN = {F32: "f32", BF16: "bf16", F16: "f16"}
DTYPES = (F32, BF16, F16)

# launch_f8's instantiations: name fragment, BN (channels) x BM (pixels) of a workgroup's tile
T0, T1, T2, FA, FB = "<64,2,2,2,2>", "<64,2,2,1,4>", "<64,2,1,1,4>", "<64,1,1,2,2>", "<64,1,1,1,4>"
TILE_DIMS = {T0: (128, 128), T1: (64, 256), T2: (64, 128), FA: (64, 64), FB: (32, 128)}

# shape: (B, H, W, Cin, Cout, kh, kw, stride, pad).  frag: the tile the launch name must show.  opts: options set around the launches.
Case = collections.namedtuple("Case", "shape frag opts maker")


def C(shape, frag, maker="int", **opts):
    return Case(tuple(shape), frag, tuple(sorted(opts.items())), maker)


def case_id(c):
    o = ",".join("%s=%s" % kv for kv in c.opts)
    return "%s%s%s" % ("x".join(str(v) for v in c.shape), "-" + o if o else "", "" if c.maker == "int" else "-" + c.maker)


def _forced_cases():
    out = []
    # F8_TILE = 0 / 1 / 2 force the three large tiles (Cout = 128); 3 matches none of them, so the launch falls through to the 64 x 64
    # tile (Cout % 64 == 0) or the 32 x 128 one (Cout = 96 / 32)
    for tile, frag, cout in ((0, T0, 128), (1, T1, 128), (2, T2, 128), (3, FA, 64), (3, FB, 96)):
        bn, bm = TILE_DIMS[frag]
        out.append(C((2, 17, 13, 64, cout, 3, 3, 2, 1), frag, F8_TILE=tile))          # M = 126: less than one pixel tile; nine K steps
        out.append(C((2, 17, 13, 128, cout, 3, 3, 1, 1), frag, F8_TILE=tile))         # M = 442: pixel tails of 58 / 186 / 58; 18 K steps
        out.append(C((1, 16, 16, 64, cout, 1, 1, 2, 0), frag, F8_TILE=tile))          # one K step: the prologue without advance()
        out.append(C((2, 9, 11, 128, cout, 1, 1, 1, 0), frag, F8_TILE=tile))          # two K steps
        # workgroup remap gidx = (blockIdx & 7) * chunk + (blockIdx >> 3) on a grid rounded up to 8: fewer than 8 tiles, exactly 8,
        # and more than 8 that are no multiple of 8 (1x1, 64 input channels; the last pixel tile lacks 37 pixels)
        if frag == FB:
            xcd = ((96, 2), (32, 8), (96, 3))                  # 3 channel tiles: 6 and 9 tiles; exactly 8 with one channel tile (Cout = 32)
        elif cout // bn == 2:
            xcd = ((cout, 3), (cout, 4), (cout, 5))            # 2 channel tiles: 6, 8, 10 tiles
        else:
            xcd = ((cout, 3), (cout, 8), (cout, 11))
        for co, mtiles in xcd:
            out.append(C((1, 1, mtiles * bm - 37, 64, co, 1, 1, 1, 0), frag, F8_TILE=tile))
    return out


def _library_cases():
    out = [
        # launch_f8's thresholds, one case per branch (1x1, 64 input channels: one MFMA step per tile)
        C((1, 256, 256, 64, 128, 1, 1, 1, 0), T0),            # blocks(128,128) = 512
        C((1, 362, 362, 64, 64, 1, 1, 1, 0), T1),             # blocks(64,256) = 512 (131044 pixels)
        C((1, 182, 182, 64, 64, 1, 1, 1, 0), T2),             # blocks(64,256) = 130, blocks(64,128) = 259 >= 256
        C((1, 209, 209, 64, 192, 1, 1, 1, 0), T1),            # 192 channels: no 128-channel tile; blocks(64,256) = 171 * 3 = 513
    ]
    # shapes of the accepted ABI that the product never sends (kh, kw in 1..7 independently, any pad), on the library's tile
    for (H, W, kh, kw, s, p) in ((9, 11, 1, 3, 1, 0), (9, 11, 1, 3, 1, 1), (11, 9, 3, 1, 1, 0), (11, 13, 5, 5, 1, 2), (13, 11, 5, 5, 2, 2),
                                 (9, 10, 7, 7, 1, 3), (15, 13, 7, 7, 2, 3), (9, 11, 3, 3, 1, 0), (9, 11, 3, 3, 1, 2), (10, 9, 3, 3, 2, 0)):
        out.append(C((2, H, W, 64, 64, kh, kw, s, p), FA))
    # operand ranges: e4m3 subnormals, and both ends of the range in both operands
    out.append(C((2, 17, 13, 128, 128, 3, 3, 1, 1), T2, "subnormal", F8_TILE=2))
    out.append(C((2, 17, 13, 128, 128, 3, 3, 2, 1), T0, "fullrange", F8_TILE=0))
    return out


CONV_CASES = _forced_cases() + _library_cases()


# ================================================================================================ convolution runner
def _u8_guarded(shape):
    """A guarded uint8 tensor (R.guarded fills with NaN, so it is made as fp32 and viewed as bytes)."""
    n = 1
    for s in shape:
        n *= int(s)
    assert n % 4 == 0
    buf, chk = R.guarded((n // 4,), torch.float32)
    return buf.view(torch.uint8).view(tuple(shape)), chk


def _scalar(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device="cuda")


def _launch(dt, d, shape, shift, res, relu, y, y8, xamax, y8amax, y8cur):
    H = pkg("_hip")
    B, Hh, W, Cin, Cout, kh, kw, s, p = shape
    Ho, Wo = R.out_size(Hh, kh, s, p), R.out_size(W, kw, s, p)
    H.call("dcf_conv2d_fwd_fp8", dt, d["x8d"], d["w8d"], d["wsd"], xamax, shift, res, y, y8, y8amax, y8cur, B, Hh, W, Cin, Ho, Wo, Cout,
           kh, kw, s, p, int(relu), H.stream_ptr())


def _assert_bytes(got, want, what, nan_ok=None):
    got, want = got.cpu(), want.cpu()
    if nan_ok is not None:                                    # either NaN code is accepted where a NaN is expected
        assert bool(((got[nan_ok] & 0x7F) == 0x7F).all()), what + ": NaN expected, got %s" % sorted(set(got[nan_ok].tolist()))[:8]
        got, want = got.clone(), want.clone()
        got[nan_ok] = 0
        want[nan_ok] = 0
    if not torch.equal(got, want):
        pytest.fail(R.report_mismatch(got.to(torch.int32), want.to(torch.int32), what), pytrace=False)


def _assert_slots(cur, want_max, what):
    cur = cur.cpu()
    assert float(cur.max()) == want_max and float(cur.min()) >= 0.0, "%s: slots hold max %r, expected %r" % (what, float(cur.max()), want_max)


def _device_operands(d):
    d = dict(d)
    d.update(x8d=d["x8"].cuda(), w8d=d["w8"].cuda(), wsd=d["wscale"].float().cuda())
    return d


def _run_conv(c, dt):
    B, Hh, W, Cin, Cout, kh, kw, s, p = c.shape
    Ho, Wo = R.out_size(Hh, kh, s, p), R.out_size(W, kw, s, p)
    tdt = R.TORCH_DT[dt]
    ref, plain, fused = F8.conv_reference(c.shape, dt, c.maker)
    d = _device_operands(ref)
    shift, res = d["shift"].float().cuda(), d["res"].to(tdt).cuda()
    # the plain call's image takes the tensor's own maximum as "the previous step's" (nothing saturates) and records no maxima; the
    # fused call's takes a sixteenth of it (the upper part of the image saturates)
    am1, am2 = F8.y8_amax(plain, dt, False), F8.y8_amax(fused, dt, True)
    want1, sy1, _ = F8.expect_y8(plain, dt, am1)
    want2, sy2, max2 = F8.expect_y8(fused, dt, am2)
    assert float((F8.stored(plain, dt).abs() * sy1).max()) <= 448.0 < float((F8.stored(fused, dt) * sy2).max())
    oshape = (B, Ho, Wo, Cout)
    y1, chk1 = R.guarded(oshape, tdt)
    y2, chk2 = R.guarded(oshape, tdt)
    i1, chk3 = _u8_guarded(oshape)
    i2, chk4 = _u8_guarded(oshape)
    cur = torch.zeros(64, dtype=torch.float32, device="cuda")
    xam = _scalar(F8.XAMAX)
    with _options(c.opts) as o:
        _launch(dt, d, c.shape, None, None, False, y1, i1, xam, _scalar(am1), None)
        _launch(dt, d, c.shape, shift, res, True, y2, i2, xam, _scalar(am2), cur)
    _assert_launches(o.names, "conv_fwd_fp8", c.frag, 2)
    chk1("plain y"); chk2("fused y"); chk3("plain y8"); chk4("fused y8")
    _assert_bits(y1, plain, dt, "plain y (n, h, w, c)")
    _assert_bits(y2, fused, dt, "fused y (n, h, w, c)")
    _assert_bytes(i1, want1, "plain y8 (n, h, w, c)")
    _assert_bytes(i2, want2, "fused y8 (n, h, w, c)")
    _assert_slots(cur, max2, "fused y8cur")


@pytest.mark.parametrize("dt", DTYPES, ids=[DTN[d] for d in DTYPES])
@pytest.mark.parametrize("case", CONV_CASES, ids=[case_id(c) for c in CONV_CASES])
def test_conv_fp8_exact(case, dt):
    _run_conv(case, dt)


NULL_SHAPE = (2, 17, 13, 64, 64, 3, 3, 2, 1)


@pytest.mark.parametrize("dt", DTYPES, ids=[DTN[d] for d in DTYPES])
def test_conv_fp8_null_scales_mean_one(dt):
    """xamax null and y8amax null: scale 1 on both; y8 null: no image, no maxima."""
    tdt = R.TORCH_DT[dt]
    ref, _, _ = F8.conv_reference(NULL_SHAPE, dt)
    d = _device_operands(ref)
    acc = ref["lin"] * ref["sx"]                              # the image's values taken at scale 1
    plain = acc * ref["wscale"].view(1, 1, 1, -1)
    fused = torch.relu(plain + ref["shift"].view(1, 1, 1, -1) + ref["res"])
    want8 = F8.encode_tensor(F8.stored(fused, dt))
    y1, chk1 = R.guarded(plain.shape, tdt)
    y2, chk2 = R.guarded(plain.shape, tdt)
    i2, chk3 = _u8_guarded(plain.shape)
    cur = torch.full((64,), 0.25, dtype=torch.float32, device="cuda")
    with _options(()) as o:
        _launch(dt, d, NULL_SHAPE, None, None, False, y1, None, None, None, cur)
        _launch(dt, d, NULL_SHAPE, d["shift"].float().cuda(), d["res"].to(tdt).cuda(), True, y2, i2, None, None, None)
    _assert_launches(o.names, "conv_fwd_fp8", FA, 2)
    chk1("plain y"); chk2("fused y"); chk3("fused y8")
    _assert_bits(y1, plain, dt, "plain y (n, h, w, c)")
    _assert_bits(y2, fused, dt, "fused y (n, h, w, c)")
    _assert_bytes(i2, want8, "fused y8 (n, h, w, c)")
    assert bool((cur == 0.25).all()), "y8cur touched although y8 is null"


NAN_SHAPE = (2, 17, 13, 64, 128, 3, 3, 2, 1)
NAN_AT = (1, 7, 6, 37)              # (b, h, w, c): odd h -> two output rows read it, even w -> one output column


@pytest.mark.parametrize("dt", DTYPES, ids=[DTN[d] for d in DTYPES])
def test_conv_fp8_nan_geometry(dt):
    """One e4m3 NaN in x8: y is NaN at exactly the pixels whose window covers it, in every channel, and bit-equal to the clean
    result elsewhere; the image y8 carries a NaN code there; y8cur is the largest finite |y|.  A ReLU epilogue is max(v, 0): it
    returns 0 for the NaN, like the 16-bit kernels."""
    B, Hh, W, Cin, Cout, kh, kw, s, p = NAN_SHAPE
    Ho, Wo = R.out_size(Hh, kh, s, p), R.out_size(W, kw, s, p)
    tdt = R.TORCH_DT[dt]
    ref, _, fused = F8.conv_reference(NAN_SHAPE, dt)
    pre = ref["lin"] * ref["wscale"].view(1, 1, 1, -1) + ref["shift"].view(1, 1, 1, -1) + ref["res"]
    d = _device_operands(ref)
    b0, h0, w0, c0 = NAN_AT
    d["x8d"][b0, h0, w0, c0] = F8.NAN_CODE
    rows = [oh for oh in range(Ho) if any(oh * s - p + i == h0 for i in range(kh))]
    cols = [ow for ow in range(Wo) if any(ow * s - p + j == w0 for j in range(kw))]
    assert (rows, cols) == ([3, 4], [3])
    hit = torch.zeros((B, Ho, Wo, Cout), dtype=torch.bool)
    for oh in rows:
        for ow in cols:
            hit[b0, oh, ow, :] = True
    shift, res = d["shift"].float().cuda(), d["res"].to(tdt).cuda()
    clean_max = float(F8.stored(pre, dt)[~hit].abs().max())
    am = F8.y8_amax(pre, dt, False)
    want8, _, _ = F8.expect_y8(pre, dt, am)
    want8r, _, _ = F8.expect_y8(torch.where(hit, torch.zeros_like(fused), fused), dt, am)
    y1, chk1 = R.guarded(pre.shape, tdt)
    y2, chk2 = R.guarded(pre.shape, tdt)
    i1, chk3 = _u8_guarded(pre.shape)
    i2, chk4 = _u8_guarded(pre.shape)
    cur1 = torch.zeros(64, dtype=torch.float32, device="cuda")
    cur2 = torch.zeros(64, dtype=torch.float32, device="cuda")
    xam = _scalar(F8.XAMAX)
    _launch(dt, d, NAN_SHAPE, shift, res, False, y1, i1, xam, _scalar(am), cur1)
    _launch(dt, d, NAN_SHAPE, shift, res, True, y2, i2, xam, _scalar(am), cur2)
    torch.cuda.synchronize()
    chk1("y"); chk2("y (ReLU)"); chk3("y8"); chk4("y8 (ReLU)")
    got = y1.cpu()
    assert bool(torch.isnan(got[hit]).all()), "%d of %d covered outputs are not NaN" % (int((~torch.isnan(got[hit])).sum()), int(hit.sum()))
    assert not bool(torch.isnan(got[~hit]).any()), "NaN outside the covered pixels"
    want = R.expect_bits(pre, dt)
    gb = R.bits_of(got).clone()
    gb[hit], want[hit] = 0, 0
    if not torch.equal(gb, want):
        pytest.fail(R.report_mismatch(gb, want, "y beside the NaN pixels (n, h, w, c)"), pytrace=False)
    _assert_bytes(i1, want8, "y8 (n, h, w, c)", nan_ok=hit)
    _assert_slots(cur1, clean_max, "y8cur")
    _assert_bits(y2, torch.where(hit, torch.zeros_like(fused), fused), dt, "y after ReLU (n, h, w, c)")
    _assert_bytes(i2, want8r, "y8 after ReLU (n, h, w, c)")
    _assert_slots(cur2, float(F8.stored(fused, dt)[~hit].abs().max()), "y8cur after ReLU")


# ================================================================================================ scale rule
def test_host_scale_rule_is_the_exact_rule():
    ops = pkg("ops")
    bad = [(a, ops.fp8_act_scale(a), F8.act_scale_exact(a)) for a in F8.scale_rule_values() if ops.fp8_act_scale(a) != F8.act_scale_exact(a)]
    assert not bad, "%d values differ, e.g. (amax, library, rule) %s" % (len(bad), bad[:6])


def _cast(dt, x, amax_prev, cur):
    H = pkg("_hip")
    x8, chk = _u8_guarded(tuple(x.shape))
    H.call("dcf_cast_fp8", dt, x, x8, _scalar(amax_prev), cur, x.numel(), H.stream_ptr())
    torch.cuda.synchronize()
    chk("x8")
    return x8


@pytest.mark.parametrize("k", [0, 1, 7, -3, 60, -100, -120, 126, 133])
def test_device_scale_equals_the_exact_rule(k):
    """amax_prev = 224 * 2^-k and its fp32 neighbours: the scale the cast kernel derives on the device, read back through the image of
    the probe values {1, 1.5, -1.75} / s, is the rule's s (k = 133: the cap 2^126)."""
    import math
    a0 = F8.f32(math.ldexp(224.0, -k))
    for amax in (F8.f32_next(a0, -1), a0, F8.f32_next(a0, 1)):
        s = F8.act_scale_exact(amax)
        probe = torch.tensor([1.0, 1.5, -1.75, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64) / s
        assert torch.equal(probe.float().double(), probe) and float(probe[0]) >= F8.FLT_MIN
        x8 = _cast(F32, probe.float().cuda(), amax, None).cpu()
        got = [F8.decode(int(b)) for b in x8[:3]]
        assert got == [1.0, 1.5, -1.75], "amax %r: the image decodes to %s: device scale %r, rule %r" % (amax, got, got[0] * s, s)


# ================================================================================================ cast
SCALE_AMAX = {1.0: 224.0, 0.125: 1000.0, 16.0: 10.0}


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_cast_every_16bit_pattern(dt):
    assert all(F8.act_scale_exact(a) == s for s, a in SCALE_AMAX.items())
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(R.TORCH_DT[dt])
    xf = x.float()
    nan = torch.isnan(xf)
    finite_max = float(xf[torch.isfinite(xf)].abs().max())
    xd = x.cuda()
    for s, amax in SCALE_AMAX.items():
        cur = torch.zeros(64, dtype=torch.float32, device="cuda")
        x8 = _cast(dt, xd, amax, cur)
        want = F8.encode_tensor(xf * s)                       # (an fp32 product, like the kernel's; Inf -> +-448, NaN stays)
        _assert_bytes(x8, want, "%s patterns at scale %g (bit pattern)" % (DTN[dt], s), nan_ok=nan)
        _assert_slots(cur, finite_max, "amax_cur (largest finite magnitude)")


def test_cast_fp32_codes_midpoints_neighbours():
    vals = F8.codec_probe_values() + [0.0, -0.0]
    vals += [0.0] * (-len(vals) % 8)
    x = torch.tensor(vals, dtype=torch.float64)
    assert torch.equal(x.float().double()[~torch.isnan(x)], x[~torch.isnan(x)])
    want = torch.tensor([F8.encode(v) for v in vals], dtype=torch.uint8)
    assert torch.equal(want, F8.encode_tensor(x))
    cur = torch.zeros(64, dtype=torch.float32, device="cuda")
    x8 = _cast(F32, x.float().cuda(), None, cur)
    _assert_bytes(x8, want, "fp32 probe values (index)", nan_ok=torch.isnan(x))
    _assert_slots(cur, F8.FLT_MAX, "amax_cur")
    # the same values at scale 16 and 1/8 (products that overflow saturate, products below 2^-10 vanish with their sign)
    for s, amax in ((16.0, 10.0), (0.125, 1000.0)):
        x8 = _cast(F32, x.float().cuda(), amax, None)
        _assert_bytes(x8, F8.encode_tensor(x.float() * s), "fp32 probe values at scale %g (index)" % s, nan_ok=torch.isnan(x))


def test_cast_grid_stride_trips_and_all_slots():
    """n / 8 = 2.5 * 2048 * 256 + 77 (the workgroup cap of 2048 is reached): workgroups 0..1023 take three trips of the grid-stride
    loop, 77 threads of workgroup 1024 a third, the rest two.  Every one of the 64 slots is written; the true maximum, a negative
    value, sits in the last 8 elements."""
    n8 = 2 * 2048 * 256 + 1024 * 256 + 77
    n = n8 * 8
    g = torch.Generator().manual_seed(77)
    x = (torch.randint(-1600, 1601, (n,), generator=g, dtype=torch.int32).float() * 0.25)       # multiples of 0.25 in [-400, 400]
    x[-5] = -777.25
    true_max = 777.25
    xd = x.cuda()
    want = F8.encode_tensor(x * F8.act_scale_exact(1000.0))
    cur = torch.zeros(64, dtype=torch.float32, device="cuda")
    x8 = _cast(F32, xd, 1000.0, cur)
    _assert_bytes(x8, want, "large tensor (index)")
    c = cur.cpu()
    assert float(c.max()) == true_max and bool((c > 0).all()) and bool((c <= true_max).all()), c.tolist()
    slot = (((n8 - 1) // 256) % 2048) & 63
    assert float(c[slot]) == true_max and int((c == true_max).sum()) == 1, "the maximum is not in the slot of the last workgroup"
    # a larger value already in a slot is kept, the others are raised as before
    cur2 = torch.full((64,), 0.25, dtype=torch.float32, device="cuda")
    cur2[7] = 1e6
    _cast(F32, xd, 1000.0, cur2)
    c2 = cur2.cpu()
    keep = torch.arange(64) != 7
    assert float(c2[7]) == 1e6 and torch.equal(c2[keep], c[keep])


@pytest.mark.parametrize("amax", [1e-40, 6.5e-37, F8.FLT_MIN], ids=["1e-40", "6.5e-37", "FLT_MIN"])
def test_tiny_amax_gives_a_finite_scale(amax):
    """amax below 224 / FLT_MAX: the scale is capped at 2^126.  Zeros stay zero bits in the image (an infinite scale made them
    0 * inf = NaN), and a convolution with that xamax returns acc * wscale * 2^-126 (an infinite scale made inv_sx 0)."""
    assert F8.act_scale_exact(amax) == 2.0 ** 126
    for dt in DTYPES:
        z = torch.zeros(4096, dtype=R.TORCH_DT[dt], device="cuda")
        x8 = _cast(dt, z, amax, None)
        assert int((x8 != 0).sum()) == 0, "zero input, image bytes %s" % sorted(set(x8.cpu().tolist()))
    shape = (1, 8, 8, 64, 64, 1, 1, 1, 0)
    ref, _, _ = F8.conv_reference(shape, F32)
    d = _device_operands(ref)
    y, chk = R.guarded((1, 8, 8, 64), torch.float32)
    _launch(F32, d, shape, None, None, False, y, None, _scalar(amax), None, None)
    torch.cuda.synchronize()
    chk("y")
    assert bool(torch.isfinite(y).all())
    # channels with wscale >= 1: wscale * 2^-126 and every non-zero product are normal numbers, so the result is exact in any
    # denormal mode
    ch = ref["wscale"] >= 1.0
    want = (ref["lin"] * ref["sx"] * ref["wscale"].view(1, 1, 1, -1) * 2.0 ** -126)[..., ch]
    assert bool((want != 0).any()) and float(want[want != 0].abs().min()) >= F8.FLT_MIN
    got = y.cpu().double()[..., ch]
    assert torch.equal(got, want), "%d of %d outputs differ from acc * wscale * 2^-126" % (int((got != want).sum()), got.numel())
