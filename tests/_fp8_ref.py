"""Exact statements of the fp8 (OCP e4m3) forward path of csrc/conv_fp8.hip (test infrastructure).

Shared by tests/test_fp8_ref_host.py (CPU) and tests/test_gpu_fp8_exact.py (GPU).  Three pieces:

* an e4m3 codec in integer / Fraction arithmetic: decode(byte), encode(fp32 value) = round to nearest even on the e4m3 grid after
  saturation at +-448, and encode_tensor, the same through a table of the grid's midpoints.  Nothing here calls torch's float8
  conversion (the host test proves the two statements equal);
* act_scale_exact, the activation scale rule of include/dcf_hip.h without a floating-point division;
* convolution references on the integer method of tests/_conv_ref.py: the e4m3 images hold small exact values, the activation scale
  sx and the per-channel weight factors are powers of two, so the fp32 accumulator holds sx * conv exactly, the epilogue product
  acc * (wscale / sx) and the sums with shift and res are exact, and the ONE rounding is the store.  Expected outputs are bit
  patterns: y in f32 / bf16 / f16 and the e4m3 image y8 of y as stored.
"""
import functools
import math
import struct
from fractions import Fraction

import torch

import _conv_ref as R

F32, BF16, F16 = R.F32, R.BF16, R.F16
E4M3_MAX = 448.0
NAN_CODE = 0x7F                     # (0xFF is the other one)
FLT_MAX = 3.4028234663852886e38
FLT_MIN = 1.1754943508222875e-38   # smallest normal
FLT_TRUE_MIN = 2.0 ** -149          # smallest subnormal


def f32(v):
    """The fp32 value nearest to the Python float v, as a Python float."""
    return struct.unpack("<f", struct.pack("<f", v))[0]


def f32_next(v, n=1):
    """n fp32 steps above (n > 0) or below (n < 0) the positive fp32 value v."""
    u = struct.unpack("<I", struct.pack("<f", v))[0] + n
    return struct.unpack("<f", struct.pack("<I", u))[0]


# ---------------------------------------------------------------------------------------------------------------- e4m3 codec
def decode_fraction(b):
    """Byte -> exact value (Fraction); None for the two NaN codes.  S.EEEE.MMM, bias 7, no infinities."""
    e, m = (b >> 3) & 15, b & 7
    if e == 15 and m == 7:
        return None
    mag = Fraction(m, 512) if e == 0 else Fraction(8 + m) * Fraction(2) ** (e - 10)
    return -mag if b & 0x80 else mag


def decode(b):
    v = decode_fraction(b)
    if v is None:
        return float("nan")
    return -0.0 if b == 0x80 else float(v)


def _rne(q):
    n = q.numerator // q.denominator
    r = q - n
    return n + 1 if (r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1)) else n


def encode(v):
    """fp32 value (Python float) -> byte: saturate to +-448 (Inf included), then round to nearest even on the e4m3 grid; subnormals
    step 2^-9; the sign survives a result of zero (-0 -> 0x80); NaN -> NAN_CODE."""
    if v != v:
        return NAN_CODE
    sign = 0x80 if math.copysign(1.0, v) < 0 else 0
    a = abs(v)
    if a >= E4M3_MAX:
        return sign | 0x7E
    a = Fraction(a)
    if a < Fraction(1, 64):
        return sign | _rne(a * 512)                          # 0..8: code 8 is the smallest normal, 2^-6
    e = math.frexp(float(a))[1] - 1                          # a = 1.xxx * 2^e (a is an fp32 value: the conversion was exact)
    n = _rne(a / Fraction(2) ** (e - 3))                     # 8..16 eighths
    if n == 16:
        e, n = e + 1, 8
    return sign | ((e + 7) << 3) | (n - 8)


POS_CODES = list(range(0x7F))                                # 0 .. 448 in ascending order of value
POS_VALUES = [decode_fraction(b) for b in POS_CODES]
MIDPOINTS = [(POS_VALUES[i] + POS_VALUES[i + 1]) / 2 for i in range(len(POS_VALUES) - 1)]
_MID_T = torch.tensor([float(m) for m in MIDPOINTS], dtype=torch.float64)
assert all(Fraction(float(m)) == m and f32(float(m)) == float(m) for m in MIDPOINTS)


def encode_tensor(v):
    """encode() of every element of a float tensor (any float dtype; values must be fp32 numbers) -> uint8.  A value below
    midpoint j takes code j, above it code j + 1, on it the even one of the two."""
    v = v.double()
    a = v.abs().clamp(max=E4M3_MAX)
    lo = torch.searchsorted(_MID_T, a, right=False)          # midpoints strictly below a
    hi = torch.searchsorted(_MID_T, a, right=True)           # midpoints at or below a
    code = torch.where(hi > lo, lo + (lo & 1), lo)           # hi > lo: a is midpoint number lo
    code = torch.where(torch.isnan(v), torch.full_like(code, NAN_CODE), code)
    sign = torch.where(torch.signbit(v) & ~torch.isnan(v), 0x80, 0)
    return (code | sign).to(torch.uint8)


def decode_tensor(b):
    lut = torch.tensor([decode(i) for i in range(256)], dtype=torch.float64)
    return lut[b.long()]


def codec_probe_values():
    """Every e4m3 value, every midpoint between adjacent values, the fp32 neighbours of each midpoint, in both signs, and the
    edges of the range: the inputs on which a rounding rule can go wrong."""
    vals = [float(x) for x in POS_VALUES]
    for m in MIDPOINTS:
        m = float(m)
        vals += [m, f32_next(m, 1), f32_next(m, -1)]
    vals += [E4M3_MAX, f32_next(E4M3_MAX, 1), f32_next(E4M3_MAX, -1), 464.0, 465.0, 480.0, f32(1e30), FLT_MAX, FLT_TRUE_MIN, FLT_MIN, float("inf")]
    return vals + [-x for x in vals] + [float("nan")]


# ---------------------------------------------------------------------------------------------------------------- scale rule
SCALE_CAP_LOG2 = 126


def act_scale_exact(amax):
    """The largest power of two s <= 2^126 with amax * s <= 224; 1 when the fp32 value of amax is not positive and finite."""
    if not (amax == amax) or amax in (float("inf"), float("-inf")):
        return 1.0
    a = f32(amax) if abs(amax) <= FLT_MAX else amax
    if not (0.0 < a <= FLT_MAX):
        return 1.0
    m, e = math.frexp(a)                                      # a = m * 2^e, m in [0.5, 1); 224 = 0.875 * 2^8
    k = min((8 if m <= 0.875 else 7) - e, SCALE_CAP_LOG2)
    A = Fraction(a)
    assert A * Fraction(2) ** k <= 224 and (k == SCALE_CAP_LOG2 or A * Fraction(2) ** (k + 1) > 224)
    return math.ldexp(1.0, k)


def scale_rule_values():
    """224 * 2^-k and its fp32 neighbours at +-1..3 ulp for every k that keeps amax positive and finite, and the named edges."""
    vals = []
    for k in range(-120, 157):                               # 224 * 2^120 = 2.98e38 .. 224 * 2^-156 = 2^-149 * 1.75 (subnormal)
        a = math.ldexp(224.0, -k)
        if not (0.0 < a <= FLT_MAX):
            continue
        a = f32(a)
        bits = struct.unpack("<I", struct.pack("<f", a))[0]
        for n in range(-3, 4):
            if 0 < bits + n <= 0x7F7FFFFF:                     # positive and finite
                vals.append(f32_next(a, n))
    vals += [FLT_TRUE_MIN, f32(1e-40), FLT_MIN, f32(6.5e-37), f32(6.6e-37), f32(1.2e-38), f32(2.9e38), f32(3.0e38), FLT_MAX,
             1e-30, 0.013, 0.5, 1.0, 3.7, 223.9, 224.0, 224.1, 448.0, 1e4,
             0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")]
    return vals


# ---------------------------------------------------------------------------------------------------------------- conv references
XAMAX = 100.0                       # "the previous step's" maximum of x: sx = 2
# amplitude of the shift (multiples of 0.5 up to +-AMP) that makes the 16-bit stores of the fused form round
AMP = {F32: 300, BF16: 300, F16: 3000}
MAKERS = ("int", "subnormal", "fullrange")


def _f32_exact(t):
    return torch.equal(t.to(torch.float32).double(), t)


@functools.lru_cache(maxsize=2)
def operands(shape, maker="int"):
    """-> dict: ximg / w (fp64, the values the e4m3 images hold), x8 / w8 (their bytes), wscale (fp64 [Cout], powers of two from
    {0.5, 1, 2, 4}; "subnormal": times 2^9), sx, lin = conv(ximg / sx, w) (fp64, exact).  The accumulator sx * lin is asserted exact
    in fp32."""
    B, H, W, Cin, Cout, kh, kw, s, p = shape
    K = kh * kw * Cin
    sx = act_scale_exact(XAMAX)
    assert sx == 2.0
    if maker == "int":
        d = R.make_fwd(shape, BF16)
        ximg, w = d["x"] * sx, d["w"]                        # image values up to +-6, weights up to +-2
        unit, bound = 1.0, 12 * K
    elif maker == "subnormal":
        ximg = R.ints((B, H, W, Cin), -7, 7, 5000) * 2.0 ** -9   # the e4m3 subnormals (and zero)
        w = R.ints((Cout, kh, kw, Cin), -2, 2, 5001)
        unit, bound = 2.0 ** -9, 14 * K
    else:
        # the ends of the e4m3 range in both operands: large x meets small w on the even input channels, small x meets large w on
        # the odd ones, so that every product is +-7, +-6.5 or 0 and every partial sum a multiple of 0.5
        big = torch.tensor([0.0, 448.0, -448.0, 416.0, -416.0], dtype=torch.float64)
        small = torch.tensor([0.0, 0.015625, -0.015625], dtype=torch.float64)
        xi_b, xi_s = torch.randint(0, 5, (B, H, W, Cin), generator=R._gen(5002)), torch.randint(0, 3, (B, H, W, Cin), generator=R._gen(5003))
        wi_b, wi_s = torch.randint(0, 5, (Cout, kh, kw, Cin), generator=R._gen(5004)), torch.randint(0, 3, (Cout, kh, kw, Cin), generator=R._gen(5005))
        even = (torch.arange(Cin) % 2 == 0)
        ximg = torch.where(even, big[xi_b], small[xi_s])
        w = torch.where(even, small[wi_s], big[wi_b])
        unit, bound = 0.5, 14 * K
    assert maker in MAKERS
    x8, w8 = encode_tensor(ximg), encode_tensor(w)
    assert torch.equal(decode_tensor(x8), ximg) and torch.equal(decode_tensor(w8), w), "the operands are not e4m3 values"
    acc = R.conv_lin(ximg, w, s, p)
    R.assert_accumulator_exact(acc / unit, bound)
    wscale = 2.0 ** (torch.randint(0, 4, (Cout,), generator=R._gen(5006)).double() - 1.0)
    if maker == "subnormal":
        wscale = wscale * 512.0                              # sums of multiples of 2^-9 brought to the range where the stores round
    return dict(ximg=ximg, w=w, x8=x8, w8=w8, wscale=wscale, sx=sx, lin=acc / sx)


@functools.lru_cache(maxsize=4)
def conv_reference(shape, dtype, maker="int"):
    """-> (inputs, exact plain result lin * wscale, exact fused result relu(lin * wscale + shift + res)).  Every intermediate of the
    epilogue (product, + shift, + res) is asserted to be an fp32 value: the store is the only rounding."""
    B, H, W, Cin, Cout, kh, kw, s, p = shape
    Ho, Wo = R.out_size(H, kh, s, p), R.out_size(W, kw, s, p)
    o = operands(shape, maker)
    shift = R.halves((Cout,), AMP[dtype], 5010)
    res = R.ints((B, Ho, Wo, Cout), -128, 128, 5011)
    plain = o["lin"] * o["wscale"].view(1, 1, 1, -1)
    t1 = plain + shift.view(1, 1, 1, -1)
    t2 = t1 + res
    assert _f32_exact(plain) and _f32_exact(t1) and _f32_exact(t2), "an epilogue term rounds in fp32"
    d = dict(o)
    d.update(shift=shift, res=res)
    return d, plain, torch.relu(t2)


def stored(exact, dtype):
    """The value of y as stored (rounded to the storage type), fp64."""
    return (exact.to(torch.float32) + 0.0).to(R.TORCH_DT[dtype]).double()


def y8_amax(exact, dtype, saturate):
    """A "previous step's" maximum for the image of y: the tensor's own maximum (nothing saturates) or a sixteenth of it (every
    |y| above 448 / sy saturates)."""
    m = float(stored(exact, dtype).abs().max())
    return f32(m / 16.0) if saturate else m


def expect_y8(exact, dtype, amax):
    """-> (bytes of encode(stored(y) * sy), sy, max |stored(y)|)."""
    sy = act_scale_exact(amax)
    st = stored(exact, dtype)
    v = st * sy
    assert _f32_exact(v)
    return encode_tensor(v), sy, float(st.abs().max())
