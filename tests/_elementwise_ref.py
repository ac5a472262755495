"""Statements of the HBM-bound kernels between the convolutions (csrc/elementwise.hip: layout conversion, cast, ReLU backward +
channel sums, the fc2 bias under the neighbour sum, bilinear resize) and the inputs that put them at their edges (test
infrastructure; CPU only: imports neither the GPU nor the library).

Layout and cast are a permutation and ONE round-to-nearest-even store: the statement is torch's conversion on the CPU and the
comparison is by raw bits (bits(), same_bits(): a NaN equals any NaN, everything else bit for bit -- the sign of a zero included).
The masked ReLU gradient is a select, where(y > 0, gy, +0.0), compared the same way.

Every sum comes with its number of terms n and the sum of their absolute values A, for tests/_fusion_ref.py::bound():
an fp32 sum of n terms lies within 1.01 * (n + 8) * 2^-24 * A + ulp_store * |want| of the fp64 value.

Resize: resize_scale and src_index are restated in fp32 with numpy float32 operations (i0, i1, l per output index).  For
align_corners = 0 the source coordinate scale * (o + 0.5) - 0.5 is two fp32 roundings, or one if the compiler contracts it into a
fused multiply-add: `fused` selects which (fused: evaluated in fp64, where the product of two fp32 numbers is exact, and rounded
once).  From the index rule come the dense per-axis weight matrices Wh [Ho,Hi], Ww [Wo,Wi] with the fp32-valued weights 1 - l and
l (added where the border clamp folds i1 onto i0); the forward is Wh . x . Ww^T + add, the backward is the transpose of the SAME
matrices, Wh^T . gy . Ww -- not a second derivation.  tests/test_elementwise_ref_host.py checks all of it against ATen in fp64."""
import numpy as np
import torch

from _fusion_ref import STORE_ULP, assert_within, bound          # noqa: F401  (re-exported: the tests take them from here)

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": 0, "bf16": 1, "f16": 2}                        # DCF_F32 / DCF_BF16 / DCF_F16
_IDT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
SMALLEST_SUBNORMAL = {torch.float32: 2.0 ** -149, torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}

# (Hi, Wi) -> (Ho, Wo), for each alignment: production's own pair (the second with an odd output), identity, degenerate sizes, the
# backward's match list exactly full (x3: six matches) and overflowing (x3.5: seven, the fallback loop), x8 / x16 / x16.5 with
# different factors on the two axes, downsampling
RESIZE_SHAPES = (((12, 39), (24, 78)), ((24, 78), (47, 156)),
                 ((5, 7), (5, 7)),
                 ((1, 1), (9, 7)), ((9, 7), (1, 1)), ((2, 3), (1, 1)), ((1, 5), (1, 5)),
                 ((4, 5), (12, 15)), ((4, 4), (14, 14)),
                 ((4, 3), (32, 48)), ((2, 3), (33, 17)), ((6, 4), (48, 64)),
                 ((20, 30), (9, 13)), ((21, 16), (3, 2)), ((8, 8), (1, 3)))
LARGE_FACTOR_SHAPES = (((4, 3), (32, 48)), ((2, 3), (33, 17)), ((6, 4), (48, 64)))      # a factor of 8 or more on some axis


# ---------------------------------------------------------------------------------------------------------------- bits
def bits(t):
    """The raw bit pattern of a floating tensor, as a CPU integer tensor of the same width."""
    t = t.detach().cpu().contiguous()
    return t.view(_IDT[t.dtype])


def same_bits(got, want, what):
    """got == want bit for bit, except that a NaN equals any NaN (the payload is not compared)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s against %s %s" % (what, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    gn, wn = torch.isnan(got), torch.isnan(want)
    bad = (gn != wn) | (~wn & (bits(got) != bits(want)))
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; element %d got %r (bits %#x) want %r (bits %#x)" % (
            what, int(bad.sum()), bad.numel(), i, float(got.reshape(-1)[i]), int(bits(got).reshape(-1)[i]) & 0xffffffff,
            float(want.reshape(-1)[i]), int(bits(want).reshape(-1)[i]) & 0xffffffff))


# ---------------------------------------------------------------------------------------------------------------- value table
def value_table():
    """fp32 values at which a conversion can go wrong, both signs of each: zeros, infinities, NaN, the largest finite values of the
    three types, fp16's overflow threshold from both sides (65519 rounds to 65504, 65520 -- the midpoint -- and 65536 to inf), the
    smallest subnormals of the three types, 2^-25 (fp16: a tie between 0 and 2^-24, to zero) and 3 * 2^-25 (a tie, to 2^-23), and
    midpoints between adjacent bf16 / fp16 values whose lower neighbour has an even / an odd mantissa (ties to even go down / up)."""
    pos = [0.0, float("inf"), 3.4028234663852886e38, 3.3895313892515355e38, 65504.0, 65519.0, 65520.0, 65536.0,
           2.0 ** -24, 2.0 ** -133, 2.0 ** -149, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -126,
           1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -11, 1 + 2.0 ** -10 + 2.0 ** -11,
           2.0 ** -134, 3 * 2.0 ** -134]                           # bf16 subnormal ties: to zero, and up to 2^-132
    t = torch.tensor(pos + [-v for v in pos] + [float("nan")], dtype=torch.float64).to(torch.float32)
    assert torch.equal(t[:len(pos)].double(), torch.tensor(pos, dtype=torch.float64)), "a table value is not an fp32 number"
    return t


def table_census(x):
    """How many elements of the fp32 tensor x fall into each class the table is there for."""
    b = bits(x.float()).to(torch.int64) & 0xffffffff
    mag, sign = b & 0x7fffffff, b >> 31
    a = x.float().abs().double()
    expo = (mag >> 23) & 0xff
    bf_tie = (mag & 0xffff) == 0x8000                                                # exactly between two bf16 values
    h_tie = ((mag & 0x1fff) == 0x1000) & (expo >= 113) & (expo <= 142)              # ... two normal fp16 values
    fin = torch.isfinite(x)
    return {
        "+0": int(((mag == 0) & (sign == 0)).sum()), "-0": int(((mag == 0) & (sign == 1)).sum()),
        "+inf": int((x == float("inf")).sum()), "-inf": int((x == float("-inf")).sum()), "nan": int(torch.isnan(x).sum()),
        "f32_max": int((a == 3.4028234663852886e38).sum()), "f16_max": int((a == 65504.0).sum()),
        "below_f16_overflow": int((a == 65519.0).sum()), "f16_overflow_tie": int((a == 65520.0).sum()), "above_f16_overflow": int((a == 65536.0).sum()),
        "f16_subnormal": int((a == 2.0 ** -24).sum()), "bf16_subnormal": int((a == 2.0 ** -133).sum()), "f32_subnormal": int((a == 2.0 ** -149).sum()),
        "f16_tie_to_zero": int((a == 2.0 ** -25).sum()),
        "bf16_tie_even": int((fin & bf_tie & (((mag >> 16) & 1) == 0) & (expo > 0)).sum()), "bf16_tie_odd": int((fin & bf_tie & (((mag >> 16) & 1) == 1) & (expo > 0)).sum()),
        "f16_tie_even": int((fin & h_tie & (((mag >> 13) & 1) == 0)).sum()), "f16_tie_odd": int((fin & h_tie & (((mag >> 13) & 1) == 1)).sum()),
    }


def table_tensor(shape, seed):
    """fp32 tensor of `shape`: the table (rotated by the seed, cut where the tensor is smaller) scattered over random values in +-4
    by a fixed permutation."""
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(1000 + seed)
    tab = value_table()
    tab = torch.roll(tab, seed % len(tab))
    x = (torch.rand(n, generator=g) * 8 - 4).float()
    k = min(n, len(tab))
    x[torch.randperm(n, generator=g)[:k]] = tab[:k]
    return x.reshape(shape)


# ---------------------------------------------------------------------------------------------------------------- layout and cast
def nchw_to_nhwc_statement(x, dtype):
    """x [B,C,H,W] fp32 -> [B,H,W,C] of dtype: a permutation and one round-to-nearest-even store."""
    return x.detach().cpu().permute(0, 2, 3, 1).contiguous().to(dtype)


def nhwc_to_nchw_statement(x):
    """x [B,H,W,C] of any storage type -> [B,C,H,W] fp32 (every value of the 16-bit types is an fp32 value)."""
    return x.detach().cpu().permute(0, 3, 1, 2).contiguous().to(torch.float32)


def cast_statement(x, dtype):
    return x.detach().cpu().to(dtype)


def image_statement(img, dtype):
    """img uint8 [B,3,H,W] -> [B,H+6,W+8,4] of dtype: float32(u8) / float32(255) in fp32, then the store; the pixel (h, w) sits at
    (h + 3, w + 3), everything else -- the halo of 3, the 2 further columns of the pitch W + 8, the fourth channel -- is +0.0."""
    a = img.detach().cpu().numpy()
    assert a.dtype == np.uint8 and a.shape[1] == 3
    B, _, H, W = a.shape
    v = a.astype(np.float32) / np.float32(255)
    assert v.dtype == np.float32
    out = np.zeros((B, H + 6, W + 8, 4), dtype=np.float32)
    out[:, 3:3 + H, 3:3 + W, :3] = v.transpose(0, 2, 3, 1)
    return torch.from_numpy(out).to(dtype)


def image_interior_mask(B, H, W):
    m = torch.zeros((B, H + 6, W + 8, 4), dtype=torch.bool)
    m[:, 3:3 + H, 3:3 + W, :3] = True
    return m


# ---------------------------------------------------------------------------------------------------------------- ReLU family
def relu_mask_statement(gy, y):
    """where(y > 0, gy, +0.0) in gy's storage type: a select (ATen's threshold backward), not a product -- a masked inf or NaN
    comes out +0.0, a masked negative gradient +0.0 and not -0.0, a kept one keeps its bits."""
    gy, y = gy.detach().cpu(), y.detach().cpu()
    return torch.where(y.float() > 0, gy, torch.zeros((), dtype=gy.dtype))


def chansum_statement(g, cnt, init):
    """init + sum over the pixels of cnt[p] * g[p, c] in fp64 -> (want [C], n, A [C]): n = npix + 1 (what the buffer held on entry
    is one more term), A = sum |cnt * g| + |init|.  cnt None: every pixel counts once."""
    g64 = g.detach().cpu().double()
    g64 = g64.reshape(-1, g64.shape[-1])
    if cnt is not None:
        g64 = g64 * cnt.detach().cpu().double().reshape(-1, 1)
    init = torch.as_tensor(init, dtype=torch.float64)
    return g64.sum(0) + init, g64.shape[0] + 1, g64.abs().sum(0) + init.abs()


def rowscale_bias_fwd_statement(y, cnt, b2):
    """y [npix,C] + cnt [npix] * b2 [C] in fp64 -> (want, n = 2, A = |y| + |cnt * b2|)."""
    y64 = y.detach().cpu().double()
    t = cnt.detach().cpu().double().reshape(-1, 1) * b2.detach().cpu().double().reshape(1, -1)
    return y64 + t, 2, y64.abs() + t.abs()


def chan_stride(npix, C, kthreads):
    """(V, cgroups, nvec, stride) of the channel-sum kernels' grid-stride walk with CHANSUM_KTHREADS = kthreads (the host side of
    csrc/elementwise.hip, chan_stride): V channels per thread, nvec vectors, `stride` threads of which each walks e, e + stride, ..."""
    V = 8 if C % 8 == 0 else 4
    cg = C // V
    nvec = npix * cg
    want = max(min(nvec, kthreads * 1024), cg)
    return V, cg, nvec, want // cg * cg


# ---------------------------------------------------------------------------------------------------------------- resize
def resize_scale(n_in, n_out, align):
    """resize_scale of csrc/elementwise.hip, an fp32 number."""
    if align:
        return np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    return np.float32(n_in) / np.float32(n_out)


def src_index(n_in, n_out, align, fused=False):
    """src_index of csrc/elementwise.hip for every output index at once -> (i0, i1 int64 [n_out], l fp32 [n_out])."""
    scale = resize_scale(n_in, n_out, align)
    o = np.arange(n_out, dtype=np.float32)
    if align:
        s = scale * o
    else:
        if fused:
            s = (np.float64(scale) * (o.astype(np.float64) + 0.5) - 0.5).astype(np.float32)      # the product is exact in fp64
        else:
            s = scale * (o + np.float32(0.5)) - np.float32(0.5)
        s = np.maximum(s, np.float32(0))
    assert s.dtype == np.float32
    i0 = np.minimum(s.astype(np.int64), n_in - 1)                  # (int)s truncates; s >= 0
    i1 = i0 + (i0 < n_in - 1)
    l = s - i0.astype(np.float32)
    assert l.dtype == np.float32
    return i0, i1, l


def resize_matrix(n_in, n_out, align, fused=False):
    """W [n_out, n_in] fp64: row o holds the fp32-valued weights 1 - l at i0 and l at i1, added where i0 == i1."""
    i0, i1, l = src_index(n_in, n_out, align, fused)
    h = np.float32(1) - l
    assert h.dtype == np.float32
    W = np.zeros((n_out, n_in), dtype=np.float64)
    r = np.arange(n_out)
    np.add.at(W, (r, i0), h.astype(np.float64))
    np.add.at(W, (r, i1), l.astype(np.float64))
    return torch.from_numpy(W)


def resize_matrices(in_hw, out_hw, align, fused=False):
    return resize_matrix(in_hw[0], out_hw[0], align, fused), resize_matrix(in_hw[1], out_hw[1], align, fused)


def resize_fwd_statement(x, out_hw, align, fused=False, add=None):
    """x [B,Hi,Wi,C] (+ add [B,Ho,Wo,C]) -> (Wh . x . Ww^T + add in fp64, n = 5, A = |Wh| . |x| . |Ww|^T + |add|)."""
    x64 = x.detach().cpu().double()
    Wh, Ww = resize_matrices(x64.shape[1:3], out_hw, align, fused)
    want = torch.einsum("oh,bhwc,pw->bopc", Wh, x64, Ww)
    A = torch.einsum("oh,bhwc,pw->bopc", Wh.abs(), x64.abs(), Ww.abs())
    if add is not None:
        a64 = add.detach().cpu().double()
        want, A = want + a64, A + a64.abs()
    return want, 5, A


def resize_bwd_statement(gy, in_hw, align, fused=False):
    """gy [B,Ho,Wo,C] -> (Wh^T . gy . Ww in fp64, n, A = |Wh|^T . |gy| . |Ww|): the transpose of the forward's matrices.  n = the
    largest number of output rows that sample one input row x the same for the columns."""
    g64 = gy.detach().cpu().double()
    Wh, Ww = resize_matrices(in_hw, g64.shape[1:3], align, fused)
    want = torch.einsum("oh,bopc,pw->bhwc", Wh, g64, Ww)
    A = torch.einsum("oh,bopc,pw->bhwc", Wh.abs(), g64.abs(), Ww.abs())
    n = int((Wh != 0).sum(0).max()) * int((Ww != 0).sum(0).max())
    return want, n, A


def resize_bwd_window(n_in, n_out, align, fixed=True):
    """The candidate window of k_resize_bwd restated in fp32: (lo, hi) int64 [n_in], the output indices input index i is searched
    in; under align_corners = 0 its upper end is floor((i + 1.5) * inv - 0.5) + 2.  fixed=False: the window before the half-pixel
    fix, whose upper end ceil((i + 1) * inv) + 2 -- still the one under align_corners = 1 -- falls short of the outputs
    o < (i + 1.5) * inv - 0.5 that reach i under align_corners = 0 once inv >= 8."""
    scale = resize_scale(n_in, n_out, align)
    inv = np.float32(1) / scale if scale > 0 else np.float32(n_out)
    i = np.arange(n_in, dtype=np.float32)
    lo = np.floor((i - np.float32(1)) * inv).astype(np.int64) - 2
    if fixed and not align:
        hi = np.floor((i + np.float32(1.5)) * inv - np.float32(0.5)).astype(np.int64) + 2
    else:
        hi = np.ceil((i + np.float32(1)) * inv).astype(np.int64) + 2
    return np.maximum(lo, 0), np.minimum(hi, n_out - 1)


def assert_one_variant(got, unfused, fused, store_dtype, what):
    """got within the bound of the unfused statement at EVERY element, or of the fused one at every element (one compile, hence one
    variant; mixing the two element by element is not allowed).  Each statement is (want, n, A).  Returns the variant that held,
    'either' where the two statements hold together."""
    held, errs = [], []
    for name, (want, n, A) in (("unfused", unfused), ("fused", fused)):
        try:
            assert_within(got, want, n, A, store_dtype, "%s [%s]" % (what, name))
            held.append(name)
        except AssertionError as e:
            errs.append(str(e))
    assert held, "%s: within the bound of neither statement -- %s" % (what, " | ".join(errs))
    return held[0] if len(held) == 1 else "either"
