"""fp64 statements of the convolution family, integer input makers and exact-bit helpers (test infrastructure).

Shared by tests/test_conv_ref_host.py (CPU) and tests/test_gpu_conv_exact.py (GPU).  The statements are plain tap loops over
shifted slices in the library's layouts: activations NHWC, forward weights [Cout][kh][kw][Cin], input-gradient weights
[Cin][kh][kw][Cout], weight gradients [Cout][kh][kw][Cin].  Nothing here calls a library convolution.

The method: with small integer inputs every product and every partial sum of a convolution is an integer below 2^24, so an fp32
accumulator holds the exact sum whatever the summation order, tiling or split.  The epilogue terms (shift in multiples of 0.5,
integer residuals) keep the fp32 sum exact too, and the ONE rounding of the result is the store to the 16-bit type -- whose
outcome, round to nearest even, is unique: the expected output is a bit pattern, not a neighbourhood.
"""
import functools

import torch

F32, BF16, F16 = 0, 1, 2
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
INT_VIEW = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}
SIG_BITS = {F32: 24, BF16: 8, F16: 11}          # significand bits of the storage types (hidden bit included)
ACC_LIMIT = float(1 << 24)                       # integers below this are exact in an fp32 accumulator
# amplitude of the epilogue terms that make the 16-bit stores round (multiples of 0.5 up to +-AMP); fp32 uses the bf16 amplitude
AMP = {F32: 300, BF16: 300, F16: 3000}
# the input gradient's residuals must be storage-representable themselves, so only sums that leave their binade can round: a wider
# amplitude (coarser residual grid against the integer gradient) is what makes 8% of the masked outputs inexact there
DGRAD_AMP = {F32: 1000, BF16: 1000, F16: 8000}


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


# ---------------------------------------------------------------------------------------------------------------- statements
def _pad_hw(x, pad):
    B, H, W, C = x.shape
    xp = torch.zeros((B, H + 2 * pad, W + 2 * pad, C), dtype=x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    return xp


def conv_lin(x, w, stride, pad):
    """x [B,H,W,Cin], w [Cout,kh,kw,Cin] (fp64) -> conv [B,Ho,Wo,Cout]."""
    assert x.dtype == torch.float64 and w.dtype == torch.float64
    B, H, W, Cin = x.shape
    Cout, kh, kw, _ = w.shape
    Ho, Wo = out_size(H, kh, stride, pad), out_size(W, kw, stride, pad)
    xp = _pad_hw(x, pad)
    y = torch.zeros((B, Ho, Wo, Cout), dtype=torch.float64)
    for i in range(kh):
        for j in range(kw):
            xs = xp[:, i:i + (Ho - 1) * stride + 1:stride, j:j + (Wo - 1) * stride + 1:stride]
            y += xs @ w[:, i, j, :].t()
    return y


def conv_fwd(x, w, stride, pad, shift=None, rowscale=None, res=None, relu=False):
    """y = act(conv + rowscale[m] * shift[c] + res); rowscale [B*Ho*Wo] or None (= 1)."""
    y = conv_lin(x, w, stride, pad)
    if shift is not None:
        s = shift.double().view(1, 1, 1, -1)
        y = y + (s if rowscale is None else rowscale.double().view(y.shape[0], y.shape[1], y.shape[2], 1) * s)
    if res is not None:
        y = y + res.double()
    return torch.relu(y) if relu else y


def dgrad_lin(gy, wt, in_hw, stride, pad):
    """gy [B,Ho,Wo,Cout], wt [Cin,kh,kw,Cout] (fp64) -> gx [B,H,W,Cin]."""
    assert gy.dtype == torch.float64 and wt.dtype == torch.float64
    B, Ho, Wo, Cout = gy.shape
    Cin, kh, kw, _ = wt.shape
    H, W = in_hw
    assert Ho == out_size(H, kh, stride, pad) and Wo == out_size(W, kw, stride, pad)
    gp = torch.zeros((B, H + 2 * pad, W + 2 * pad, Cin), dtype=torch.float64)
    for i in range(kh):
        for j in range(kw):
            gp[:, i:i + (Ho - 1) * stride + 1:stride, j:j + (Wo - 1) * stride + 1:stride] += gy @ wt[:, i, j, :].t()
    return gp[:, pad:pad + H, pad:pad + W].contiguous()


def conv_dgrad(gy, wt, in_hw, stride, pad, res=None, resq=None, mask=None):
    """gx = (dgrad + res + scatter(resq)) * (mask > 0); resq lives on the (2i, 2j) sub-grid of gx."""
    gx = dgrad_lin(gy, wt, in_hw, stride, pad)
    if res is not None:
        gx = gx + res.double()
    if resq is not None:
        gx[:, ::2, ::2] += resq.double()
    if mask is not None:
        gx = torch.where(mask.double() > 0, gx, torch.zeros_like(gx))      # (a select: the zeros are +0, as the kernels store them)
    return gx


def conv_wgrad(x, gy, kh, kw, stride, pad):
    """x [B,H,W,Cin], gy [B,Ho,Wo,Cout] (fp64) -> (G [Cout,kh,kw,Cin], column sums of gy [Cout])."""
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = gy.shape
    assert Ho == out_size(H, kh, stride, pad) and Wo == out_size(W, kw, stride, pad)
    return wgrad_taps(_pad_hw(x, pad), gy, kh, kw, stride)


def wgrad_taps(xp, gy, kh, kw, stride):
    """The same on an input that carries its padding already (the stem's NHWC4 + halo image): tap (i, j) of output pixel (oh, ow)
    reads xp[oh * stride + i, ow * stride + j]."""
    assert xp.dtype == torch.float64 and gy.dtype == torch.float64
    _, Ho, Wo, Cout = gy.shape
    Cin = xp.shape[3]
    g2 = gy.reshape(-1, Cout)
    G = torch.zeros((Cout, kh, kw, Cin), dtype=torch.float64)
    for i in range(kh):
        for j in range(kw):
            xs = xp[:, i:i + (Ho - 1) * stride + 1:stride, j:j + (Wo - 1) * stride + 1:stride]
            G[:, i, j, :] = g2.t() @ xs.reshape(-1, Cin)
    return G, g2.sum(0)


# ---------------------------------------------------------------------------------------------------------------- input makers
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def ints(shape, lo, hi, seed):
    """Integers in [lo, hi] as fp64."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).double()


def halves(shape, amp, seed):
    """Multiples of 0.5 in [-amp, amp] as fp64."""
    return torch.randint(-2 * amp, 2 * amp + 1, tuple(shape), generator=_gen(seed)).double() * 0.5


def storable(t, dtype):
    """The values of t rounded to the storage type (so that the tensor can be handed to the device unchanged), as fp64."""
    return t.to(torch.float32).to(TORCH_DT[dtype]).double()


def make_fwd(shape, dtype, seed=1000):
    """shape = (B, H, W, Cin, Cout, kh, kw, stride, pad).  x in [-3, 3], w in [-2, 2]; the fused call's shift in multiples of 0.5 up
    to +-AMP, res integers in [-128, 128], rowscale integers in 0..3."""
    B, H, W, Cin, Cout, kh, kw, s, p = shape
    Ho, Wo = out_size(H, kh, s, p), out_size(W, kw, s, p)
    return dict(x=ints((B, H, W, Cin), -3, 3, seed), w=ints((Cout, kh, kw, Cin), -2, 2, seed + 1),
                shift=halves((Cout,), AMP[dtype], seed + 2), res=ints((B, Ho, Wo, Cout), -128, 128, seed + 3),
                rowscale=ints((B * Ho * Wo,), 0, 3, seed + 4))


def make_dgrad(shape, dtype, seed=2000):
    """gy in [-3, 3], wt in [-2, 2]; res / resq storage-representable multiples of 0.5 up to +-DGRAD_AMP; mask mixed-sign integers with
    zeros (half of them positive)."""
    B, H, W, Cin, Cout, kh, kw, s, p = shape
    Ho, Wo = out_size(H, kh, s, p), out_size(W, kw, s, p)
    return dict(gy=ints((B, Ho, Wo, Cout), -3, 3, seed), wt=ints((Cin, kh, kw, Cout), -2, 2, seed + 1),
                res=storable(halves((B, H, W, Cin), DGRAD_AMP[dtype], seed + 2), dtype),
                resq=storable(halves((B, (H + 1) // 2, (W + 1) // 2, Cin), DGRAD_AMP[dtype], seed + 3), dtype),
                mask=ints((B, H, W, Cin), -1, 2, seed + 4))


def make_wgrad(shape, seed=3000):
    B, H, W, Cin, Cout, kh, kw, s, p = shape
    Ho, Wo = out_size(H, kh, s, p), out_size(W, kw, s, p)
    return dict(x=ints((B, H, W, Cin), -3, 3, seed), gy=ints((B, Ho, Wo, Cout), -3, 3, seed + 1))


def binary_image(B, H, W, seed=4000):
    """uint8 NCHW image whose bytes are only 0 and 255: x / 255.0f is exactly 0 or 1."""
    return (torch.randint(0, 2, (B, 3, H, W), generator=_gen(seed)) * 255).to(torch.uint8)


# ---- references, computed once per (shape, dtype) and shared by every case / option variant of the shape; callers must not modify them
@functools.lru_cache(maxsize=4)
def fwd_reference(shape, dtype, rowscale=False):
    """-> (inputs, exact plain conv, exact fused result: relu(conv + [rowscale *] shift + res))."""
    B, H, W, Cin, Cout, kh, kw, s, p = shape
    d = make_fwd(shape, dtype)
    lin = conv_lin(d["x"], d["w"], s, p)
    assert_accumulator_exact(lin, 6 * kh * kw * Cin)
    fused = conv_fwd(d["x"], d["w"], s, p, d["shift"], d["rowscale"] if rowscale else None, d["res"], True)
    return d, lin, fused


@functools.lru_cache(maxsize=4)
def dgrad_reference(shape, dtype, halfres=False):
    """-> (inputs, exact plain input gradient, exact fused result: (dgrad + res [+ scatter(resq)]) * (mask > 0))."""
    B, H, W, Cin, Cout, kh, kw, s, p = shape
    d = make_dgrad(shape, dtype)
    lin = dgrad_lin(d["gy"], d["wt"], (H, W), s, p)
    assert_accumulator_exact(lin, 6 * kh * kw * Cout)
    fused = conv_dgrad(d["gy"], d["wt"], (H, W), s, p, d["res"], d["resq"] if halfres else None, d["mask"])
    return d, lin, fused


@functools.lru_cache(maxsize=4)
def wgrad_reference(shape):
    """-> (inputs, exact G [Cout,kh,kw,Cin], exact column sums of gy [Cout])."""
    B, H, W, Cin, Cout, kh, kw, s, p = shape
    d = make_wgrad(shape)
    G, gs = conv_wgrad(d["x"], d["gy"], kh, kw, s, p)
    Ho, Wo = out_size(H, kh, s, p), out_size(W, kw, s, p)
    assert_accumulator_exact(G, 9 * B * Ho * Wo)
    assert_accumulator_exact(gs, 3 * B * Ho * Wo)
    return d, G, gs


def image_nhwc4(img):
    """img uint8 [B,3,H,W] -> fp64 [B,H+6,W+8,4], the layout of dcf_image_to_nhwc4: x / 255 with a halo of 3, channels padded to 4."""
    B, _, H, W = img.shape
    x4 = torch.zeros((B, H + 6, W + 8, 4), dtype=torch.float64)
    x4[:, 3:3 + H, 3:3 + W, :3] = (img.double() / 255.0).permute(0, 2, 3, 1)
    return x4


@functools.lru_cache(maxsize=4)
def stem_reference(shape, dtype):
    """shape = (B, H, W, Cout): the 7x7 / stride-2 / pad-3 stem on a 0 / 255 image.  -> (inputs, exact plain conv, exact
    relu(conv + shift), exact weight gradient in the device layout [Cout][7][8][4], exact column sums of gy)."""
    B, H, W, Cout = shape
    img = binary_image(B, H, W)
    x = (img.double() / 255.0).permute(0, 2, 3, 1).contiguous()          # exactly 0 or 1
    w = ints((Cout, 7, 7, 3), -2, 2, 4001)
    shift = halves((Cout,), AMP[dtype], 4002)
    lin = conv_lin(x, w, 2, 3)
    assert_accumulator_exact(lin, 2 * 147)
    Ho, Wo = out_size(H, 7, 2, 3), out_size(W, 7, 2, 3)
    gy = ints((B, Ho, Wo, Cout), -3, 3, 4003)
    x4 = image_nhwc4(img)
    assert torch.equal(x4[:, 3:3 + H, 3:3 + W, :3], x)
    G, gs = wgrad_taps(x4, gy, 7, 8, 2)
    assert_accumulator_exact(G, 3 * B * Ho * Wo)
    return dict(img=img, w=w, shift=shift, gy=gy), lin, conv_fwd(x, w, 2, 3, shift, None, None, True), G, gs


def assert_accumulator_exact(exact, bound):
    """`bound` = the sum of the largest magnitudes of all terms (6 per forward / input-gradient product, 9 per weight-gradient
    product, 3 per gy term): every partial sum, in any order, is an integer of at most that size, and it is exact in fp32."""
    assert bound < ACC_LIMIT, "the integer sums may leave the exact range of fp32"
    assert float(exact.abs().max()) <= bound and bool((exact == exact.round()).all())


# ---------------------------------------------------------------------------------------------------------------- exact bits
def expect_bits(exact, dtype):
    """fp64 -> fp32 (asserted lossless) -> storage type by torch's round-to-nearest-even conversion -> integer bit pattern."""
    f = exact.to(torch.float32)
    assert torch.equal(f.double(), exact), "the exact result is not an fp32 value"
    f = f + 0.0                                      # (-0 -> +0: a sum or a select never produces the negative zero)
    return f.to(TORCH_DT[dtype]).contiguous().view(INT_VIEW[dtype])


def bits_of(t):
    """Integer view of a device or host tensor of a storage type."""
    return t.contiguous().view({torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}[t.dtype])


def census(exact, dtype):
    """Fractions of the outputs that (a) are not representable in the storage type, (b) lie exactly half way between two storage
    values, (c) are non-zero (survived the ReLU / mask).  Normal range only (our magnitudes are >= 0.5 or zero)."""
    v = exact.abs().flatten()
    nz = v > 0
    m, e = torch.frexp(v[nz])                       # v = m * 2^e, m in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(m), e - SIG_BITS[dtype])
    frac = torch.remainder(v[nz] / ulp, 1.0)
    n = float(v.numel())
    return float((frac != 0).sum()) / n, float((frac == 0.5).sum()) / n, float(nz.sum()) / n


def assert_census(exact, dtype, what):
    """The conditions under which a fused 16-bit case tests the store's rounding at all (on the reference alone)."""
    inexact, ties, alive = census(exact, dtype)
    assert inexact >= 0.08, "%s: only %.1f%% of the outputs need rounding" % (what, 100 * inexact)
    assert ties >= 0.04, "%s: only %.1f%% of the outputs are exact ties" % (what, 100 * ties)
    assert 0.30 <= alive <= 0.70, "%s: %.1f%% of the outputs survive the ReLU / mask" % (what, 100 * alive)
    return inexact, ties, alive


# ---------------------------------------------------------------------------------------------------------------- guarded buffers
GUARD_BYTES = 64 * 1024
GUARD_BYTE = 0xA5
# include/dcf_hip.h: the tensors of the convolution entries are 16-byte aligned (nothing more): the view starts 16 bytes past a
# 32-byte boundary
MIN_ALIGN = 16


def guarded(shape, dtype, device="cuda"):
    """A contiguous NaN-filled tensor of `dtype` (torch dtype) inside a larger allocation whose margins (>= 64 KiB on both sides)
    hold a sentinel byte; the view is offset by the minimum alignment the header states.  -> (view, check) where check() asserts
    that no byte of either margin has changed."""
    es = torch.empty((), dtype=dtype).element_size()
    n = 1
    for s in shape:
        n *= int(s)
    nbytes = n * es
    lead = GUARD_BYTES + MIN_ALIGN                   # torch allocations are 512-byte aligned: lead = 16 (mod 32)
    tail = GUARD_BYTES + (-(lead + nbytes)) % 16
    raw = torch.full((lead + nbytes + tail,), GUARD_BYTE, dtype=torch.uint8, device=device)
    view = raw[lead:lead + nbytes].view(dtype).view(tuple(shape))
    view.fill_(float("nan"))
    assert view.data_ptr() % MIN_ALIGN == 0 and view.data_ptr() % (2 * MIN_ALIGN) != 0

    def check(what="output"):
        before, after = raw[:lead], raw[lead + nbytes:]
        nb, na = int((before != GUARD_BYTE).sum()), int((after != GUARD_BYTE).sum())
        assert nb == 0 and na == 0, "%s: %d bytes written before and %d bytes after the tensor" % (what, nb, na)

    return view, check


def report_mismatch(got_bits, want_bits, what, limit=6):
    """Count of wrong elements and the first few (n, h, w, c, got, want) of a 4-D comparison (any rank works)."""
    got_bits, want_bits = got_bits.cpu(), want_bits.cpu()
    bad = (got_bits != want_bits).nonzero()
    lines = ["%s: %d of %d elements differ" % (what, bad.shape[0], got_bits.numel())]
    for idx in bad[:limit].tolist():
        t = tuple(idx)
        lines.append("  %s got 0x%x want 0x%x" % (t, int(got_bits[t]) & 0xFFFFFFFF, int(want_bits[t]) & 0xFFFFFFFF))
    return "\n".join(lines)
