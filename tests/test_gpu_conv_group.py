"""Grouped launches of independent implicit-GEMM convolutions (dcf_conv2d_fwd_group / dcf_conv2d_dgrad_group, csrc/conv.hip).

Every grouped call is compared in two ways: with the same items through the single-layer entry points, bit for bit, and with the
exact integer statements of tests/_conv_ref.py (small-integer inputs: every partial sum is exact in fp32, the one rounding is the
16-bit store, so the expected output is a bit pattern).  Outputs live in NaN-filled guarded buffers.  Every case asserts the launch
names the profiling layer recorded: a case that silently fell back to single launches (or grouped what it must not) fails.

Launch names: conv_fwd_grp_<dt><KB,TN,TM,WN,WM[,db|,dmaN]> / conv_dgrad_grp_...; the tile and the ring depth follow the per-layer
rule of launch_igemm, ",db" / the LDS-DMA form (<= 512 workgroups) is decided on the launch's TOTAL workgroup count.
"""
import ctypes
import functools

import pytest
import torch

import _conv_ref as R
from _util import pkg

pytestmark = pytest.mark.gpu

F32, BF16, F16 = R.F32, R.BF16, R.F16
DTN = {F32: "f32", BF16: "bf16", F16: "f16"}
DTS = [BF16, F16]
DT_IDS = ["bf16", "f16"]


# ================================================================================================ members and their exact results
@functools.lru_cache(maxsize=None)
def fwd_member(shape, dt, seed, xseed=None, shift=True, res=False, relu=False):
    """shape = (B, H, W, Cin, Cout, kh, kw, stride, pad); members with the same xseed and input shape read the same x."""
    B, Hh, W, Cin, Cout, kh, kw, s, p = shape
    Ho, Wo = R.out_size(Hh, kh, s, p), R.out_size(W, kw, s, p)
    x = R.ints((B, Hh, W, Cin), -3, 3, seed if xseed is None else xseed)
    w = R.ints((Cout, kh, kw, Cin), -2, 2, seed + 1)
    sh = R.halves((Cout,), R.AMP[dt], seed + 2) if shift else None
    rs = R.ints((B, Ho, Wo, Cout), -128, 128, seed + 3) if res else None
    R.assert_accumulator_exact(R.conv_lin(x, w, s, p), 6 * kh * kw * Cin)
    return dict(kind="fwd", shape=shape, dt=dt, x=x, w=w, shift=sh, res=rs, relu=relu, oshape=(B, Ho, Wo, Cout),
                exact=R.conv_fwd(x, w, s, p, sh, None, rs, relu))


@functools.lru_cache(maxsize=None)
def dgrad_member(shape, dt, seed, res=False, mask=False):
    """shape as above, H x W the size of gx; Cout = the reduction channels, Cin = the produced ones."""
    B, Hh, W, Cin, Cout, kh, kw, s, p = shape
    Ho, Wo = R.out_size(Hh, kh, s, p), R.out_size(W, kw, s, p)
    gy = R.ints((B, Ho, Wo, Cout), -3, 3, seed)
    wt = R.ints((Cin, kh, kw, Cout), -2, 2, seed + 1)
    rs = R.storable(R.halves((B, Hh, W, Cin), R.DGRAD_AMP[dt], seed + 2), dt) if res else None
    mk = R.ints((B, Hh, W, Cin), -1, 2, seed + 4) if mask else None
    R.assert_accumulator_exact(R.dgrad_lin(gy, wt, (Hh, W), s, p), 6 * kh * kw * Cout)
    return dict(kind="dgrad", shape=shape, dt=dt, gy=gy, wt=wt, res=rs, mask=mk, oshape=(B, Hh, W, Cin),
                exact=R.conv_dgrad(gy, wt, (Hh, W), s, p, rs, None, mk))


def conv1x1(B, Hh, W, Cin, Cout):
    return (B, Hh, W, Cin, Cout, 1, 1, 1, 0)


# ================================================================================================ runner
def _dev(t, dt):
    return None if t is None else t.to(R.TORCH_DT[dt]).cuda().contiguous()


class _options:
    """Options set around the launches and reset afterwards; the launch names recorded meanwhile."""

    def __init__(self, opts):
        self.opts, self.names = tuple(sorted(opts.items())), {}

    def __enter__(self):
        H = pkg("_hip")
        for k, v in self.opts:
            H.set_option(k, v)
        H.call("dcf_prof_reset")
        H.call("dcf_prof_enable", 1)
        return self

    def __exit__(self, *exc):
        H = pkg("_hip")
        try:
            torch.cuda.synchronize()
            H.call("dcf_prof_enable", 0)
            self.names = {n: v[1] for n, v in H.prof_read().items()}
        finally:
            H.call("dcf_prof_enable", 0)
            H.call("dcf_prof_reset")
            for k, _ in self.opts:
                H.set_option(k, None)
        return False


def _run(members, opts, want):
    """want: {launch name: count} -- exactly the conv_fwd* / conv_dgrad* launches the grouped call must make."""
    H = pkg("_hip")
    kind = members[0]["kind"]
    assert all(m["kind"] == kind for m in members)
    st, n = H.stream_ptr(), len(members)
    keep, outs_g, outs_s, checks = [], [], [], []
    for m in members:
        dt = m["dt"]
        if kind == "fwd":
            t = dict(x=_dev(m["x"], dt), w=_dev(m["w"], dt), shift=None if m["shift"] is None else m["shift"].float().cuda(), res=_dev(m["res"], dt))
        else:
            t = dict(gy=_dev(m["gy"], dt), wt=_dev(m["wt"], dt), res=_dev(m["res"], dt), mask=_dev(m["mask"], dt))
        keep.append(t)
        for outs in (outs_g, outs_s):
            y, chk = R.guarded(m["oshape"], R.TORCH_DT[dt])
            outs.append(y)
            checks.append(chk)
    ptr = lambda t: None if t is None else t.data_ptr()
    if kind == "fwd":
        items = (H.ConvFwdItem * n)()
        for i, (m, t) in enumerate(zip(members, keep)):
            B, Hh, W, Cin, Cout, kh, kw, s, p = m["shape"]
            items[i] = H.ConvFwdItem(m["dt"], 1 if m["relu"] else 0, ptr(t["x"]), ptr(t["w"]), ptr(t["shift"]), ptr(t["res"]), outs_g[i].data_ptr(),
                                     B, Hh, W, Cin, m["oshape"][1], m["oshape"][2], Cout, kh, kw, s, p, 0)
        entry, base = "dcf_conv2d_fwd_group", "conv_fwd"
    else:
        items = (H.ConvDgradItem * n)()
        for i, (m, t) in enumerate(zip(members, keep)):
            B, Hh, W, Cin, Cout, kh, kw, s, p = m["shape"]
            items[i] = H.ConvDgradItem(m["dt"], 0, ptr(t["gy"]), ptr(t["wt"]), ptr(t["res"]), ptr(t["mask"]), outs_g[i].data_ptr(),
                                       B, Hh, W, Cin, R.out_size(Hh, kh, s, p), R.out_size(W, kw, s, p), Cout, kh, kw, s, p, 0)
        entry, base = "dcf_conv2d_dgrad_group", "conv_dgrad"
    with _options(opts) as o:
        H.call(entry, ctypes.addressof(items), n, st)
    got = {k: c for k, c in o.names.items() if k.startswith(base)}
    assert got == want, "launches of the grouped call: %s, expected %s" % (sorted(got.items()), sorted(want.items()))
    # the same items through the single-layer entry points (same options, so the per-layer rule picks the same tiles)
    single_opts = dict(opts)
    single_opts.pop("IGEMM_GROUP", None)
    with _options(single_opts) as o1:
        for i, (m, t) in enumerate(zip(members, keep)):
            B, Hh, W, Cin, Cout, kh, kw, s, p = m["shape"]
            if kind == "fwd":
                H.call("dcf_conv2d_fwd", m["dt"], t["x"], t["w"], t["shift"], t["res"], outs_s[i], B, Hh, W, Cin, m["oshape"][1], m["oshape"][2], Cout,
                       kh, kw, s, p, 1 if m["relu"] else 0, st)
            else:
                H.call("dcf_conv2d_dgrad", m["dt"], t["gy"], t["wt"], t["res"], t["mask"], outs_s[i], B, Hh, W, Cin, R.out_size(Hh, kh, s, p),
                       R.out_size(W, kw, s, p), Cout, kh, kw, s, p, st)
    assert not any("_grp" in k for k in o1.names), o1.names
    for chk in checks:
        chk()
    for i, m in enumerate(members):
        gb, sb = R.bits_of(outs_g[i]), R.bits_of(outs_s[i])
        if not torch.equal(gb, sb):
            pytest.fail(R.report_mismatch(gb, sb, "member %d: grouped against single launch (n, h, w, c)" % i), pytrace=False)
        want_bits = R.expect_bits(m["exact"], m["dt"]).cuda()
        if not torch.equal(gb, want_bits):
            pytest.fail(R.report_mismatch(gb, want_bits, "member %d: grouped against the exact statement (n, h, w, c)" % i), pytrace=False)


def grp(kind, dt, tail):
    return "conv_%s_grp_%s<%s>" % (kind, DTN[dt], tail)


def one(kind, dt, tail):
    return "conv_%s_%s<%s>" % (kind, DTN[dt], tail)


# ================================================================================================ the sites' shapes
def _head(dt, ck, cn, seed):
    """A strided block's first two layers on one 2x17x13 input: the 1x1 / stride-2 shortcut and the 3x3 / stride-2 conv1 (ReLU)."""
    return [fwd_member((2, 17, 13, ck, cn, 1, 1, 2, 0), dt, seed, xseed=seed + 50),
            fwd_member((2, 17, 13, ck, cn, 3, 3, 2, 1), dt, seed + 10, xseed=seed + 50, relu=True)]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("ck,cn,tail", [(32, 64, "64,1,1,2,2,db"), (64, 128, "128,1,1,2,2,dma4")], ids=["32to64", "64to128"])
def test_stage_head_pair(dt, ck, cn, tail):
    # M = 2*9*7 = 126 pixels: two pixel tiles of 64, the second with 62 live rows; 32 channels = 64-byte K chunks (register staging)
    _run(_head(dt, ck, cn, 100 + ck), {}, {grp("fwd", dt, tail): 1})


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_stage_head_pair_register_form(dt):
    """IGEMM_DMA=0: the 128-byte-chunk launch takes the register-staged kernel with two LDS buffers."""
    _run(_head(dt, 64, 128, 164), {"IGEMM_DMA": 0}, {grp("fwd", dt, "128,1,1,2,2,db"): 1})


LAT_HW = [(24, 78), (12, 39), (6, 20), (3, 10)]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_four_laterals_of_different_sizes(dt):
    # 59, 15, 4 and 1 workgroups (none a multiple of 8; the last member is a single, partly filled tile); with a residual on one
    ms = [fwd_member(conv1x1(2, h, w, ck, 64), dt, 200 + ck, res=(ck == 128)) for (h, w), ck in zip(LAT_HW, (64, 128, 256, 512))]
    _run(ms, {}, {grp("fwd", dt, "128,1,1,2,2,dma4"): 1})


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_three_laterals_with_192_channels(dt):
    # Cn = 192 = three 64-channel tiles: 177 + 45 + 12 workgroups
    ms = [fwd_member(conv1x1(2, h, w, ck, 192), dt, 300 + ck) for (h, w), ck in zip(LAT_HW, (128, 192, 256))]
    _run(ms, {}, {grp("fwd", dt, "128,1,1,2,2,dma4"): 1})


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_shared_input_members(dt):
    # one [1, 300, 1, 64] input (300 = 4 * 64 + 44 pixels), Cn 64 / 128 / 192 / 256: at this size the per-layer rule gives every
    # member (192 = 3 * 64 included) the 64x64 tile, so all four share one launch
    ms = [fwd_member(conv1x1(1, 300, 1, 64, cn), dt, 400 + cn, xseed=450, shift=(cn != 128)) for cn in (64, 128, 192, 256)]
    _run(ms, {}, {grp("fwd", dt, "128,1,1,2,2,dma4"): 1})


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_shared_input_members_fall_into_two_buckets(dt):
    # the same four on 8320 pixels: Cn 256 reaches 256 workgroups with 64x128 tiles and is alone in its bucket; the other three
    # (130 + 260 + 390 workgroups of 64x64) share a launch of more than 512 workgroups (register staging, one LDS buffer)
    ms = [fwd_member(conv1x1(1, 8320, 1, 64, cn), dt, 1400 + cn, xseed=1450, relu=(cn == 192)) for cn in (64, 128, 192, 256)]
    _run(ms, {}, {grp("fwd", dt, "128,1,1,2,2"): 1, one("fwd", dt, "128,2,1,1,4,dma3"): 1})


def _dgrads(dt, n):
    spec = [((24, 78), 64, 64, False, False), ((12, 39), 128, 128, True, False), ((6, 20), 256, 64, True, True), ((3, 10), 64, 256, False, False)]
    return [dgrad_member(conv1x1(2, h, w, cin, cout), dt, 500 + 10 * i, res=r, mask=m) for i, ((h, w), cin, cout, r, m) in enumerate(spec[:n])]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("n", [3, 4])
def test_input_gradients(dt, n):
    _run(_dgrads(dt, n), {}, {grp("dgrad", dt, "128,1,1,2,2,dma4"): 1})


# ================================================================================================ the launches of more than 512 workgroups
# (the forms the benchmark-size groups take: register staging, one LDS buffer)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_large_group_64x64_tiles(dt):
    ms = [fwd_member(conv1x1(2, 24, 78, ck, 256), dt, 600 + ck) for ck in (64, 128, 192)]          # 3 x 236 workgroups
    _run(ms, {}, {grp("fwd", dt, "128,1,1,2,2"): 1})


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_large_group_64x128_tiles(dt):
    ms = [fwd_member(conv1x1(2, 52, 80, ck, 192), dt, 700 + ck) for ck in (64, 128, 192)]          # TILE=1: 3 x 195 workgroups
    _run(ms, {"TILE": 1}, {grp("fwd", dt, "128,2,1,1,4"): 1})


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_large_group_128x128_tiles(dt):
    ms = [fwd_member(conv1x1(2, 52, 80, 64, 256), dt, 800 + i, xseed=850) for i in range(4)]       # TILE=0: 4 x 130 workgroups
    _run(ms, {"TILE": 0}, {grp("fwd", dt, "128,2,2,2,2"): 1})


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_large_group_64_byte_chunks(dt):
    ms = [fwd_member(conv1x1(2, 52, 80, 32, 128), dt, 900 + i, xseed=950, relu=(i == 1)) for i in range(4)]   # TILE=1: 4 x 130 workgroups
    _run(ms, {"TILE": 1}, {grp("fwd", dt, "64,2,1,1,4"): 1})


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_large_group_of_input_gradients(dt):
    ms = [dgrad_member(conv1x1(2, 24, 78, 256, co), dt, 1000 + co, res=(co == 128), mask=(co == 64)) for co in (64, 128, 192)]   # 3 x 236
    _run(ms, {}, {grp("dgrad", dt, "128,1,1,2,2"): 1})


# ================================================================================================ edges
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_group_of_one_is_the_single_launch(dt):
    _run([fwd_member(conv1x1(2, 12, 39, 128, 64), dt, 328, res=True)], {}, {one("fwd", dt, "128,1,1,2,2,dma4"): 1})
    _run(_dgrads(dt, 1), {}, {one("dgrad", dt, "128,1,1,2,2,dma4"): 1})


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("n", [5, 9])
def test_more_members_than_one_launch_holds(dt, n):
    # 4 per launch: n = 5 -> one group and a single launch, n = 9 -> two groups and a single launch
    ms = [fwd_member(conv1x1(1, 5 + 3 * i, 7, 64, 64), dt, 1100 + 7 * i, relu=(i % 2 == 1)) for i in range(n)]
    _run(ms, {}, {grp("fwd", dt, "128,1,1,2,2,dma4"): n // 4, one("fwd", dt, "128,1,1,2,2,dma4"): 1})


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_members_that_must_fall_back_inside_a_group(dt):
    H = pkg("_hip")
    # forward: a 3x3 / stride-1 64-channel layer (the streaming / row-sharing kernels' layer) and an fp32 item between two 1x1 members
    ms = [fwd_member(conv1x1(2, 12, 39, 128, 64), dt, 328, res=True),
          fwd_member((2, 12, 39, 64, 64, 3, 3, 1, 1), dt, 1200),
          fwd_member(conv1x1(1, 6, 20, 64, 64), F32, 1210),
          fwd_member(conv1x1(2, 6, 20, 256, 64), dt, 1220, relu=True)]
    st = H.stream_ptr()
    m = ms[1]                        # (the name the 3x3 layer's own kernel reports: asked from the library, not restated here)
    t = dict(x=_dev(m["x"], dt), w=_dev(m["w"], dt), shift=m["shift"].float().cuda())
    y = torch.empty(m["oshape"], dtype=R.TORCH_DT[dt], device="cuda")
    with _options({}) as o:
        H.call("dcf_conv2d_fwd", dt, t["x"], t["w"], t["shift"], None, y, 2, 12, 39, 64, 12, 39, 64, 3, 3, 1, 1, 0, st)
    (name3x3,) = [k for k in o.names if k.startswith("conv_fwd")]
    assert "_grp" not in name3x3
    _run(ms, {}, {grp("fwd", dt, "128,1,1,2,2,dma4"): 1, name3x3: 1, one("fwd", F32, "128,1,1,2,2,db"): 1})
    # input gradients: a 3x3 / stride-2 layer (parity classes) between two 1x1 members
    md = [_dgrads(dt, 2)[0], dgrad_member((2, 17, 13, 64, 64, 3, 3, 2, 1), dt, 1230, res=True, mask=True), _dgrads(dt, 2)[1]]
    _run(md, {}, {grp("dgrad", dt, "128,1,1,2,2,dma4"): 1, one("dgrad", dt, "128,1,1,2,2,dma4"): 1})


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_option_igemm_group_off(dt):
    ms = [fwd_member(conv1x1(2, h, w, ck, 64), dt, 200 + ck, res=(ck == 128)) for (h, w), ck in zip(LAT_HW, (64, 128, 256, 512))]
    _run(ms, {"IGEMM_GROUP": 0}, {one("fwd", dt, "128,1,1,2,2,dma4"): 4})
    _run(_dgrads(dt, 3), {"IGEMM_GROUP": 0}, {one("dgrad", dt, "128,1,1,2,2,dma4"): 3})
