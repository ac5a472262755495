"""Every convolution kernel variant against exact integer statements (tests/_conv_ref.py), bit for bit.

Inputs are small integers, so every partial sum is an integer below 2^24 and the fp32 accumulators are exact in any order; the
epilogue terms are chosen so that the 16-bit stores have to round.  Forward and input gradient: the output must be
RNE_storage(exact) in every bit.  Weight gradient: slabs.sum(0) and gsum.sum(0) must equal the fp64 sums.  No tolerances.

Every case names the options it sets and a fragment of the launch name the library's profiling layer must report: a case that
silently took another kernel fails.  Outputs live in guarded buffers (NaN-filled, 16 bytes past a 32-byte boundary, 64 KiB of
sentinel bytes on either side).  The tables are read by tests/test_conv_ref_host.py too, which asserts on the references alone
that the fused 16-bit cases do round (>= 8% inexact outputs, >= 4% exact ties, 30-70% alive after the ReLU / mask).

Shapes are the smallest that reach their branch; the comments next to the tables say which lines of the dispatch code decide.
"""
import collections

import pytest
import torch

import _conv_ref as R
from _util import pkg

pytestmark = pytest.mark.gpu

F32, BF16, F16 = R.F32, R.BF16, R.F16
DTN = {F32: "f32", BF16: "bf16", F16: "f16"}

# kind: fwd | rowscale | dgrad | halfres | wgrad | stem_fwd | stem_wgrad.  shape: (B, H, W, Cin, Cout, kh, kw, stride, pad), H x W the
# size of x / gx (stem: (B, H, W, Cout)).  opts: the options set around the launches.  frag: what the launch name must contain.
# fused: also the fused call form (16-bit fused cases are the ones the host census covers).  nsplit: 0 = ask the library.
Case = collections.namedtuple("Case", "kind shape dtype opts frag fused nsplit")


def C(kind, shape, dtype, frag, fused=True, nsplit=0, **opts):
    return Case(kind, tuple(shape), dtype, tuple(sorted(opts.items())), frag, fused, nsplit)


def case_id(c):
    o = ",".join("%s=%s" % kv for kv in c.opts)
    return "%s-%s-%s%s%s" % (c.kind, "x".join(str(v) for v in c.shape), DTN[c.dtype], "-" + o if o else "", "-ns%d" % c.nsplit if c.nsplit else "")


def chan(kind, B, H, W, Ck, Cn, kh, kw, s, p):
    """Shape from the kernel's point of view: Ck reduction channels, Cn produced channels (the input gradient swaps the roles)."""
    return (B, H, W, Ck, Cn, kh, kw, s, p) if kind in ("fwd", "rowscale") else (B, H, W, Cn, Ck, kh, kw, s, p)


# ================================================================================================ implicit GEMM (conv.hip)
# launch_igemm: TILE forces (TN, TM, WN, WM); KB = 128 when a pixel row of Ck channels is a multiple of 128 bytes, else 64;
# ",db" = at most 512 workgroups; 16-bit KB = 128 launches take k_conv_igemm_dma (",dma<ring>") when IGEMM_DMA allows.
TILES = {0: (2, 2, 2, 2), 1: (2, 1, 1, 4), 2: (1, 1, 2, 2), 3: (1, 1, 1, 4), 4: (2, 1, 2, 2)}
# more than 512 workgroups with Cn = 128: 128x128 tiles need > 65536 pixels, 64x128 / 128x64 > 32768, 64x64 / 32x128 > 16384
BIG_HW = {0: (258, 255), 1: (182, 182), 4: (182, 182), 2: (127, 131), 3: (127, 131)}


def igemm_frag(kb, tile, tail):
    tn, tm, wn, wm = TILES[tile]
    ring = 4 if (wn * tn * 32 + wm * tm * 32) <= 128 else 3
    return "<%d,%d,%d,%d,%d%s>" % (kb, tn, tm, wn, wm, {"db": ",db", "sb": "", "dma": ",dma%d" % ring, "dma2": ",dma2"}[tail])


def _igemm_cases():
    out = []
    for kind in ("fwd", "dgrad"):
        for tile in range(5):
            small = lambda ck: chan(kind, 2, 17, 13, ck, 128, 3, 3, 2, 1)          # odd sizes, stride 2 (input gradient: parity classes)
            big = lambda ck: chan(kind, 1, BIG_HW[tile][0], BIG_HW[tile][1], ck, 128, 1, 1, 1, 0)
            for dt in (BF16, F16):
                # 64-byte rows: register-staged kernel, double- and single-buffered
                out.append(C(kind, small(32), dt, igemm_frag(64, tile, "db"), TILE=tile))
                out.append(C(kind, big(32), dt, igemm_frag(64, tile, "sb"), TILE=tile))
                # 128-byte rows: IGEMM_DMA 0 / 1 (default) / 2 / 3 on both launch sizes
                out.append(C(kind, small(64), dt, igemm_frag(128, tile, "db"), TILE=tile, IGEMM_DMA=0))
                out.append(C(kind, small(64), dt, igemm_frag(128, tile, "dma"), TILE=tile))
                out.append(C(kind, small(64), dt, igemm_frag(128, tile, "dma"), TILE=tile, IGEMM_DMA=3))
                out.append(C(kind, big(64), dt, igemm_frag(128, tile, "sb"), TILE=tile))
                out.append(C(kind, big(64), dt, igemm_frag(128, tile, "dma"), TILE=tile, IGEMM_DMA=2))
                out.append(C(kind, big(64), dt, igemm_frag(128, tile, "dma2"), TILE=tile, IGEMM_DMA=3))
            # fp32: 16 and 48 channels are 64- and 192-byte rows (KB = 64), 32 channels 128-byte rows
            out.append(C(kind, small(16), F32, igemm_frag(64, tile, "db"), TILE=tile))
            out.append(C(kind, small(48), F32, igemm_frag(64, tile, "db"), TILE=tile))
            out.append(C(kind, big(16), F32, igemm_frag(64, tile, "sb"), TILE=tile))
            out.append(C(kind, small(32), F32, igemm_frag(128, tile, "db"), TILE=tile))
            out.append(C(kind, big(32), F32, igemm_frag(128, tile, "sb"), TILE=tile))
        # the single-buffered form at a product-like width: 1x1 64 -> 64 on 1 x 182 x 182 with 32 x 128 tiles (259 x 2 workgroups)
        out.append(C(kind, chan(kind, 1, 182, 182, 64, 64, 1, 1, 1, 0), BF16, igemm_frag(128, 3, "sb"), TILE=3))
        # shapes of the accepted ABI that the product never sends (check_conv: kh, kw in 1..7 independently, any pad), tile by the
        # library's own choice: Cn = 64 -> 64x64 tiles, Cn = 32 / 96 -> 32x128
        for dt in (BF16, F16, F32):
            kb = 64 if dt == F32 else 128
            for (H, W, kh, kw, s, p) in ((9, 11, 1, 3, 1, 0), (9, 11, 1, 3, 1, 1), (11, 9, 3, 1, 1, 0), (11, 13, 5, 5, 1, 2), (13, 11, 5, 5, 2, 2),
                                         (9, 10, 7, 7, 1, 3), (15, 13, 7, 7, 2, 3), (9, 11, 3, 3, 1, 0), (9, 11, 3, 3, 1, 2), (10, 9, 3, 3, 2, 0)):
                ck = 48 if dt == F32 else 64
                out.append(C(kind, chan(kind, 2, H, W, ck, 64, kh, kw, s, p), dt, igemm_frag(kb, 2, "db" if dt == F32 else "dma")))
            # 1x1 / stride 2 on odd sizes: three quarters of gx get no gradient term, so a representable residual stays representable
            # there and the census cannot hold -- 16-bit input gradients run the plain form only (the fp32 fused form is exact anyway)
            out.append(C(kind, chan(kind, 2, 15, 11, ck, 96, 1, 1, 2, 0), dt, igemm_frag(kb, 3, "db" if dt == F32 else "dma"),
                         fused=(kind == "fwd" or dt == F32)))
    # stride 2: DGRAD_PARITY 0 (one plain pass) / 1 (parity classes) / 2 (classes only for rows of >= 128 bytes) on odd sizes
    for dt in (BF16, F16, F32):
        for (H, W) in ((17, 13), (9, 79)):
            for cn in (32, 64):                    # Cn = produced channels of gx: 64 / 128 / 256 bytes a row
                frag = igemm_frag(64 if dt == F32 else 128, 2 if cn == 64 else 3, "db" if dt == F32 else "dma")
                for par in (0, 1, 2):
                    out.append(C("dgrad", chan("dgrad", 2, H, W, 48 if dt == F32 else 64, cn, 3, 3, 2, 1), dt, frag, DGRAD_PARITY=par))
                out.append(C("halfres", chan("dgrad", 2, H, W, 48 if dt == F32 else 64, cn, 3, 3, 2, 1), dt, frag))
        out.append(C("halfres", chan("dgrad", 1, 12, 10, 32, 128, 5, 5, 2, 2), dt, igemm_frag(128 if dt == F32 else 64, 0, "db"), TILE=0))
        # dcf_conv2d_fwd_rowscale (1x1): the library's own tile and the 128x128 one
        kb = 64 if dt == F32 else 128
        out.append(C("rowscale", (2, 9, 13, 48 if dt == F32 else 64, 64, 1, 1, 1, 0), dt, igemm_frag(kb, 2, "db" if dt == F32 else "dma")))
        out.append(C("rowscale", (1, 11, 13, 48 if dt == F32 else 64, 128, 1, 1, 1, 0), dt, igemm_frag(kb, 0, "db" if dt == F32 else "dma"), TILE=0))
    return out


IGEMM_CASES = _igemm_cases()

# ================================================================================================ row-sharing kernel (conv_rs.hip)
# rs_plan: kind 0 = 128 channels x (2 waves x up to 5 position tiles), kind 1 = 64 x (4 x 3), kind 2 = 64 x (4 x 1); RS_KIND / RS_NPT
# force a pair; a wave's tile count is npt / WM rounded either way, so the pairs below reach every `switch (cnt)` arm 0..TMMAX.
# The launch name ends in ",pf>" when the rotated tap loop runs (conv_rs.hip: pf_name).
RS_PAIRS = [(0, n) for n in range(1, 11)] + [(1, n) for n in range(1, 13)] + [(2, n) for n in range(1, 5)]


def rs_frag(kind, npt, pf):
    return "<rs%d,%d%s>" % (kind, npt, ",pf" if pf else "")


def _rs_cases():
    out = []
    for kind in ("fwd", "dgrad"):
        sm = lambda k, ck=64: chan(kind, 2, 9, 21, ck, 128 if k == 0 else 64, 3, 3, 1, 1)          # 2 x 9 x 23 = 414 padded positions
        many = lambda k: chan(kind, 2, 64, 64, 64, 128 if k == 0 else 64, 3, 3, 1, 1)             # RS_NPT=1: 264 tiles for 256 workgroups
        for dt in (BF16, F16):
            for (k, n) in RS_PAIRS:
                out.append(C(kind, sm(k), dt, rs_frag(k, n, True), CONV_LC=0, RS_KIND=k, RS_NPT=n))
        for (k, n) in RS_PAIRS:
            # the plain tap loop (kind 2: the consumers' stage-granular loop off as well) in every wave-count specialisation
            out.append(C(kind, sm(k), BF16, rs_frag(k, n, False), CONV_LC=0, RS_KIND=k, RS_NPT=n, RS_PF=0))
        for n in range(1, 9):
            # kind 1 with at most eight position tiles: the DX = 1 instantiation (TMMAX = 3) instead of the DX = 2 one, both loops
            out.append(C(kind, sm(1), BF16, rs_frag(1, n, True), CONV_LC=0, RS_KIND=1, RS_NPT=n, RS_DX2=0))
            out.append(C(kind, sm(1), F16, rs_frag(1, n, False), CONV_LC=0, RS_KIND=1, RS_NPT=n, RS_DX2=0, RS_PF=0))
        for dt in (BF16, F16):
            for n in (1, 4):
                out.append(C(kind, sm(2), dt, rs_frag(2, n, False), CONV_LC=0, RS_KIND=2, RS_NPT=n, RS_S3=0))
                out.append(C(kind, sm(2), dt, rs_frag(2, n, False), CONV_LC=0, RS_KIND=2, RS_NPT=n, RS_L16=0))
                out.append(C(kind, sm(2), dt, rs_frag(2, n, False), CONV_LC=0, RS_KIND=2, RS_NPT=n, RS_PF2=0))
                out.append(C(kind, sm(2), dt, rs_frag(2, n, True), CONV_LC=0, RS_KIND=2, RS_NPT=n, RS_PF=2))
            # one to four 64-channel chunks of the reduction, on each kind
            for ck in (128, 192, 256):
                for (k, n) in ((0, 7), (1, 5), (1, 11), (2, 3)):
                    out.append(C(kind, sm(k, ck), dt, rs_frag(k, n, True), CONV_LC=0, RS_KIND=k, RS_NPT=n))
            # persistent workgroups that walk several tiles (264 tiles, 256 workgroups); 64 reduction channels and more than one
            # round: the plain loop is the default of kinds 0 / 1 there, RS_PF=2 forces the rotated one; RS_PERSIST=0: 264 workgroups
            for k in (0, 1, 2):
                out.append(C(kind, many(k), dt, rs_frag(k, 1, k == 2), CONV_LC=0, RS_KIND=k, RS_NPT=1))
                out.append(C(kind, many(k), dt, rs_frag(k, 1, k == 2), CONV_LC=0, RS_KIND=k, RS_NPT=1, RS_PERSIST=0))
                out.append(C(kind, many(k), dt, rs_frag(k, 1, True), CONV_LC=0, RS_KIND=k, RS_NPT=1, RS_PF=2))
    return out


RS_CASES = _rs_cases()

# ================================================================================================ loader / consumer kernel (conv_lc.hip)
# lc_plan: kind 0 = 128 channels, kind 1 = 64; tiles TH x TW with an even TW >= 14, TH * TW <= 320 and (TH + 2)(TW + 2) staged pixels
# within 440 (kind 0) / 504 (kind 1).  A tile has ceil(TH * TW / 32) groups dealt to two consumers: 1 / 3 / 5 / 7 / 9 / 10 groups
# give the `switch (cnt)` arms {1,0} {2,1} {3,2} {4,3} {5,4} {5,5}.


def _lc_cases():
    out = []
    for kind in ("fwd", "dgrad"):
        for dt in (BF16, F16):
            for k in (0, 1):
                cn = 128 if k == 0 else 64
                f = lambda th, tw: "<lc%d,%dx%d>" % (k, th, tw)
                # 1 x 14 (smallest) .. 22 x 14 on an odd image of two tile columns
                for th in (1, 5, 10, 15, 20, 22):
                    out.append(C(kind, chan(kind, 1, 23, 17, 64, cn, 3, 3, 1, 1), dt, f(th, 14), CONV_LC=2, LC_KIND=k, LC_TH=th, LC_TW=14))
                # the largest tile of 320 positions; kind 1 also the widest its bigger pixel slot allows (7 x 66 = 462 staged pixels)
                out.append(C(kind, chan(kind, 2, 23, 25, 64, cn, 3, 3, 1, 1), dt, f(16, 20), CONV_LC=2, LC_KIND=k, LC_TH=16, LC_TW=20))
                if k == 1:
                    out.append(C(kind, chan(kind, 1, 7, 67, 64, cn, 3, 3, 1, 1), dt, f(5, 64), CONV_LC=2, LC_KIND=k, LC_TH=5, LC_TW=64))
                # W < 14, odd sizes, one to four chunks of reduction channels; the tile is the plan's own
                for ck in (64, 128, 192, 256):
                    out.append(C(kind, chan(kind, 2, 9, 13, ck, cn, 3, 3, 1, 1), dt, "<lc%d," % k, CONV_LC=2, LC_KIND=k))
                # 320 tiles for 256 persistent workgroups
                out.append(C(kind, chan(kind, 2, 40, 56, 64, cn, 3, 3, 1, 1), dt, f(1, 14), CONV_LC=2, LC_KIND=k, LC_TH=1, LC_TW=14))
    return out


LC_CASES = _lc_cases()

# ================================================================================================ spatial-tile kernel (conv_sp.hip)
# Cin == Cout in {32, 64}; tiles of 8 x 32 (32 channels) / 4 x 32 (64 channels) pixels; CONV_SP_MIN_PIX=0 sends small launches there.


def _sp_cases():
    out = []
    for kind in ("fwd", "dgrad"):
        for dt in (BF16, F16):
            for c, th in ((32, 8), (64, 4)):
                for W in (31, 32, 33):                  # one short of / exactly / one past a tile column; heights one past a tile row
                    out.append(C(kind, (2, th + 1, W, c, c, 3, 3, 1, 1), dt, "<sp%d>" % c, CONV_SP_MIN_PIX=0))
            out.append(C(kind, (2, 9, 33, 32, 32, 3, 3, 1, 1), dt, "<sp32>", CONV_SP_MIN_PIX=0, CONV_SP_NBUF32=3))
            # one workgroup per CU and more tiles than workgroups: 3 x 9 x 10 = 270 and 2 x 11 x 12 = 264 tiles
            out.append(C(kind, (3, 72, 320, 32, 32, 3, 3, 1, 1), dt, "<sp32>", CONV_SP_MIN_PIX=0, CONV_SP_WGPC=1))
            out.append(C(kind, (2, 44, 384, 64, 64, 3, 3, 1, 1), dt, "<sp64>", CONV_SP_MIN_PIX=0, CONV_SP_WGPC=1))
    return out


SP_CASES = _sp_cases()

# ================================================================================================ stem
STEM_CASES = [C(k, (2, 22, 30, co), dt, "stem_fwd_" if k == "stem_fwd" else "stem_wgrad_")
              for k in ("stem_fwd", "stem_wgrad") for dt in (BF16, F16, F32) for co in (64, 32)]

# ================================================================================================ weight gradients
# dcf_conv2d_wgrad's routes, in its order: conv_wgv.hip (32 -> 32), conv_wgs.hip (128-multiples, W + 2 >= 40), conv_wg1.hip (1x1 and
# 3x3 / stride 2 / pad 1, 64-multiples, >= 2048 pixels), k_conv_wgrad3g (3x3 / stride 1 / pad 1, LDS-DMA: rows of >= 40 resp. 48
# padded positions), k_conv_wgrad3, and the generic k_conv_wgrad for everything else.


def _wgrad_cases():
    g, w3, w3g, wgs, wg1, wgv = [], [], [], [], [], []
    W = lambda *a, **k: C("wgrad", *a, **k)
    for dt in (BF16, F16, F32):
        n = "conv_wgrad_%s" % DTN[dt]
        lo = 48 if dt == F32 else 32                   # TN = 1: a partial (fp32: 48 of 64) or full input-channel tile
        # ---- generic kernel, the four tile pairs <TM,TN>: fewer than 2048 pixels (1x1 and 3x3 / stride 2), odd pixel counts
        for cin, cout, tm, tn in ((lo, 32, 1, 1), (lo, 96, 2, 1), (64, 32, 1, 2), (96, 96, 2, 2)):
            g.append(W((2, 9, 7, cin, cout, 1, 1, 1, 0), dt, "%s<%d,%d>" % (n, tm, tn)))
            g.append(W((1, 15, 13, cin, cout, 3, 3, 2, 1), dt, "%s<%d,%d>" % (n, tm, tn)))
        # 5x5 and 7x7, (1,3) and (3,1), pads that are not k / 2
        g.append(W((2, 11, 13, 64, 64, 5, 5, 1, 2), dt, n + "<2,2>"))
        g.append(W((1, 15, 13, 64, 32, 7, 7, 2, 3), dt, n + "<1,2>"))
        g.append(W((2, 9, 11, 64, 64, 1, 3, 1, 1), dt, n + "<2,2>"))
        g.append(W((2, 11, 9, 64, 64, 3, 1, 1, 0), dt, n + "<2,2>"))
        g.append(W((2, 9, 11, 64, 64, 3, 3, 1, 0), dt, n + "<2,2>"))
        g.append(W((2, 9, 11, 64, 64, 3, 3, 1, 2), dt, n + "<2,2>"))
        # XCD-aware mapping on (8 ranges, WGRAD_XCD_MIN=8) and off (3 ranges and 1 range) on an odd pixel count; nine taps: on from 8
        for ns, o in ((8, {"WGRAD_XCD_MIN": 8}), (8, {}), (3, {}), (1, {})):
            g.append(W((3, 19, 13, 64, 96, 1, 1, 1, 0), dt, n + "<2,2>", nsplit=ns, **o))
        for ns in (8, 3):
            g.append(W((3, 19, 13, 64, 96, 3, 3, 2, 1), dt, n + "<2,2>", nsplit=ns))
        # WGRAD3=0: the generic kernel on a 3x3 / stride-1 layer
        g.append(W((2, 9, 21, 64, 64, 3, 3, 1, 1), dt, n + "<2,2>", WGRAD3=0))
        # ---- k_conv_wgrad3: <1,1,3> is the 32 -> 32 layer (16-bit: with conv_wgv.hip off, or H / W below 8), the others take narrow rows
        n3 = "conv_wgrad3_%s" % DTN[dt]
        w3.append(W((2, 9, 21, 32, 32, 3, 3, 1, 1), dt, n3 + "<1,1,3>", WGRAD3V=0))
        w3.append(W((2, 7, 21, 32, 32, 3, 3, 1, 1), dt, n3 + "<1,1,3>"))
        w3.append(W((2, 21, 7, 32, 32, 3, 3, 1, 1), dt, n3 + "<1,1,3>"))
        w3.append(W((2, 9, 21, 32, 96, 3, 3, 1, 1), dt, n3 + "<2,1,1>"))
        w3.append(W((2, 9, 21, 96, 32, 3, 3, 1, 1), dt, n3 + "<1,2,1>"))
        # (fp32: 2 x 2 fragments do not fit the registers, the launch takes <2,1,1>)
        w3.append(W((3, 9, 37, 96, 96, 3, 3, 1, 1), dt, n3 + ("<2,1,1>" if dt == F32 else "<2,2,1>")))
        w3.append(W((2, 9, 50, 64, 64, 3, 3, 1, 1), dt, n3 + ("<2,1,1>" if dt == F32 else "<2,2,1>"), WGRAD3_DMA=0))
        w3.append(W((2, 9, 50, 32, 64, 3, 3, 1, 1), dt, n3 + "<2,1,1>", WGRAD3_DMA=0))
        w3.append(W((2, 9, 50, 64, 32, 3, 3, 1, 1), dt, n3 + "<1,2,1>", WGRAD3_DMA=0))
        if dt == F32:
            continue
        # ---- k_conv_wgrad3g: the three tile pairs, eight and four waves; rows of exactly 40 / 48 padded positions wrap once a stage;
        # three frames so that pixel ranges cross frames; WGRAD_RANGE_XCD=1; WGRAD3S=0 sends a 128 -> 128 layer here
        ng = "conv_wgrad3g_%s" % DTN[dt]
        for nw, tail in ((8, ",2,8>"), (4, ",4,4>")):
            o = {} if nw == 8 else {"WGRAD3_NW": 4}
            w3g.append(W((3, 9, 38, 64, 64, 3, 3, 1, 1), dt, ng + "<2,2" + tail, **o))
            w3g.append(W((3, 9, 46, 32, 96, 3, 3, 1, 1), dt, ng + "<2,1" + tail, **o))
            w3g.append(W((3, 9, 38, 96, 32, 3, 3, 1, 1), dt, ng + "<1,2" + tail, **o))
            w3g.append(W((2, 11, 53, 96, 160, 3, 3, 1, 1), dt, ng + "<2,2" + tail, **o))
            w3g.append(W((3, 9, 38, 64, 64, 3, 3, 1, 1), dt, ng + "<2,2" + tail, WGRAD_RANGE_XCD=1, **o))
            w3g.append(W((2, 9, 44, 128, 128, 3, 3, 1, 1), dt, ng + "<2,2" + tail, WGRAD3S=0, **o))
        # ---- conv_wgs.hip: 128 -> 128 and 256 -> 128, W + 2 = 40 and wider, frames inside ranges
        ns_ = "conv_wgrad3s_grp_%s<2,2,2,3>" % DTN[dt]
        wgs.append(W((2, 9, 38, 128, 128, 3, 3, 1, 1), dt, ns_))
        wgs.append(W((3, 21, 41, 256, 128, 3, 3, 1, 1), dt, ns_))
        wgs.append(W((3, 9, 38, 128, 128, 3, 3, 1, 1), dt, ns_, WGRAD_RANGE_XCD=1))
        # ---- conv_wg1.hip, forced small (WGRAD1S_MIN_PIXELS=1): sixteen- and eight-wave form, 25 pixels, a last tap column on the image's
        # last column (odd W, stride 2), 128-channel granule (a 64-channel layer then stays on the generic kernel)
        n1 = "conv_wgrad1s_grp_%s<4>" % DTN[dt]
        for l16 in (1, 0):
            for shp in ((1, 5, 5, 64, 64, 1, 1, 1, 0), (2, 14, 10, 64, 128, 1, 1, 2, 0), (2, 9, 7, 320, 64, 1, 1, 1, 0), (1, 9, 79, 128, 192, 3, 3, 2, 1),
                        (3, 23, 37, 64, 128, 3, 3, 2, 1)):
                wg1.append(W(shp, dt, n1, WGRAD1S_MIN_PIXELS=1, WGRAD1S_L16=l16))
        wg1.append(W((1, 9, 79, 128, 256, 3, 3, 2, 1), dt, n1, WGRAD1S_MIN_PIXELS=1, WGRAD1S_GRANULE=128))
        wg1.append(W((1, 9, 79, 128, 192, 3, 3, 2, 1), dt, n + "<2,2>", WGRAD1S_MIN_PIXELS=1, WGRAD1S_GRANULE=128))
        # the generic kernel through WGRAD1S=0, and through a pad that is not k / 2 with the split count the library names for the layer
        g.append(W((1, 9, 79, 128, 192, 3, 3, 2, 1), dt, n + "<2,2>", WGRAD1S_MIN_PIXELS=1, WGRAD1S=0))
        g.append(W((2, 21, 25, 64, 128, 3, 3, 2, 0), dt, n + "<2,2>", WGRAD1S_MIN_PIXELS=1))
        # ---- conv_wgv.hip (32 -> 32): strips of 32 columns, row ranges of >= 8 rows; few and many units
        nv = "conv_wgrad3v_%s" % DTN[dt]
        for (B, H, Wd) in ((1, 8, 8), (2, 17, 31), (2, 9, 32), (3, 25, 33)):
            for units in (None, 1, 100000):
                o = {} if units is None else {"WGRAD3V_UNITS": units}
                wgv.append(W((B, H, Wd, 32, 32, 3, 3, 1, 1), dt, nv, **o))
    return g, w3, w3g, wgs, wg1, wgv


WG_GENERIC, WG3_CASES, WG3G_CASES, WGS_CASES, WG1_CASES, WGV_CASES = _wgrad_cases()

CONV_CASES = IGEMM_CASES + RS_CASES + LC_CASES + SP_CASES
WGRAD_CASES = WG_GENERIC + WG3_CASES + WG3G_CASES + WGS_CASES + WG1_CASES + WGV_CASES


# ================================================================================================ runners
def _dev(t, dtype):
    return t.to(R.TORCH_DT[dtype]).cuda().contiguous()


class _options:
    """Options set for the launches of one case and reset to None afterwards; the launch names recorded meanwhile."""

    def __init__(self, opts):
        self.opts, self.names = opts, {}

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


def _assert_launches(names, base, frag, count):
    mine = {n: c for n, c in names.items() if n.startswith(base)}
    assert mine and all(frag in n for n in mine) and sum(mine.values()) == count, \
        "expected %d launches named %s...%s, the library reports %s" % (count, base, frag, sorted(names.items()))


def _assert_bits(got, exact, dtype, what):
    want = R.expect_bits(exact, dtype).cuda()
    got_bits = R.bits_of(got)
    if not torch.equal(got_bits, want):
        pytest.fail(R.report_mismatch(got_bits, want, what), pytrace=False)


def _run_conv(c):
    H = pkg("_hip")
    B, Hh, W, Cin, Cout, kh, kw, s, p = c.shape
    Ho, Wo = R.out_size(Hh, kh, s, p), R.out_size(W, kw, s, p)
    dt, tdt, st = c.dtype, R.TORCH_DT[c.dtype], H.stream_ptr()
    dims = (B, Hh, W, Cin, Ho, Wo, Cout, kh, kw, s, p)
    if c.kind in ("fwd", "rowscale"):
        d, lin, fused = R.fwd_reference(c.shape, dt, c.kind == "rowscale")
        x, w, shift, res = _dev(d["x"], dt), _dev(d["w"], dt), d["shift"].float().cuda(), _dev(d["res"], dt)
        rowscale = d["rowscale"].float().cuda()
        oshape, base = (B, Ho, Wo, Cout), "conv_fwd"
        if c.kind == "fwd":
            plain_exact = lin
            plain = lambda y: H.call("dcf_conv2d_fwd", dt, x, w, None, None, y, *dims, 0, st)
            full = lambda y: H.call("dcf_conv2d_fwd", dt, x, w, shift, res, y, *dims, 1, st)
        else:
            plain_exact = R.conv_fwd(d["x"], d["w"], s, p, d["shift"], d["rowscale"])
            plain = lambda y: H.call("dcf_conv2d_fwd_rowscale", dt, x, w, shift, rowscale, None, y, *dims, 0, st)
            full = lambda y: H.call("dcf_conv2d_fwd_rowscale", dt, x, w, shift, rowscale, res, y, *dims, 1, st)
    else:
        d, lin, fused = R.dgrad_reference(c.shape, dt, c.kind == "halfres")
        gy, wt, res, resq, mask = (_dev(d[k], dt) for k in ("gy", "wt", "res", "resq", "mask"))
        oshape, base = (B, Hh, W, Cin), "conv_dgrad"
        if c.kind == "dgrad":
            plain_exact = lin
            plain = lambda y: H.call("dcf_conv2d_dgrad", dt, gy, wt, None, None, y, *dims, st)
            full = lambda y: H.call("dcf_conv2d_dgrad", dt, gy, wt, res, mask, y, *dims, st)
        else:
            plain_exact = R.conv_dgrad(d["gy"], d["wt"], (Hh, W), s, p, None, d["resq"], None)
            plain = lambda y: H.call("dcf_conv2d_dgrad_halfres", dt, gy, wt, None, resq, None, y, *dims, st)
            full = lambda y: H.call("dcf_conv2d_dgrad_halfres", dt, gy, wt, res, resq, mask, y, *dims, st)
    y1, chk1 = R.guarded(oshape, tdt)
    y2, chk2 = R.guarded(oshape, tdt)
    with _options(c.opts) as o:
        plain(y1)
        if c.fused:
            full(y2)
    _assert_launches(o.names, base, c.frag, 2 if c.fused else 1)
    chk1("plain output")
    chk2("fused output")
    _assert_bits(y1, plain_exact, dt, "plain (n, h, w, c)")
    if c.fused:
        _assert_bits(y2, fused, dt, "fused (n, h, w, c)")


def _assert_sums(slabs, gsum, G, gs, what):
    assert not bool(torch.isnan(slabs).any()), what + ": slab entries left unwritten"
    got = slabs.sum(0).double().cpu()                   # integers below 2^24: the fp32 sum over the slabs is exact
    if not torch.equal(got, G):
        pytest.fail(R.report_mismatch(got.to(torch.int64), G.to(torch.int64), what + " slabs.sum(0) (co, kh, kw, ci)"), pytrace=False)
    if gsum is not None:
        assert not bool(torch.isnan(gsum).any()), what + ": gsum entries left unwritten"
        gg = gsum.sum(0).double().cpu()
        if not torch.equal(gg, gs):
            pytest.fail(R.report_mismatch(gg.to(torch.int64), gs.to(torch.int64), what + " gsum.sum(0) (co)"), pytrace=False)


def _run_wgrad(c):
    H = pkg("_hip")
    B, Hh, W, Cin, Cout, kh, kw, s, p = c.shape
    Ho, Wo = R.out_size(Hh, kh, s, p), R.out_size(W, kw, s, p)
    dt, st = c.dtype, H.stream_ptr()
    d, G, gs = R.wgrad_reference(c.shape)
    x, gy = _dev(d["x"], dt), _dev(d["gy"], dt)
    with _options(c.opts) as o:
        ns = c.nsplit or H.call("dcf_conv2d_wgrad_splits", B, Ho, Wo, Cin, Cout, kh, kw, s)
        assert ns >= 1
        slabs, chk_s = R.guarded((ns, Cout, kh, kw, Cin), torch.float32)
        gsum, chk_g = R.guarded((4 * ns, Cout), torch.float32)
        slabs0, chk_0 = R.guarded((ns, Cout, kh, kw, Cin), torch.float32)
        H.call("dcf_conv2d_wgrad", dt, x, gy, slabs, gsum, ns, B, Hh, W, Cin, Ho, Wo, Cout, kh, kw, s, p, st)
        H.call("dcf_conv2d_wgrad", dt, x, gy, slabs0, None, ns, B, Hh, W, Cin, Ho, Wo, Cout, kh, kw, s, p, st)
    _assert_launches(o.names, "conv_wgrad", c.frag, 2)
    chk_s("slabs"); chk_g("gsum"); chk_0("slabs (gsum null)")
    _assert_sums(slabs, gsum, G, gs, "with gsum")
    _assert_sums(slabs0, None, G, gs, "gsum null")
    assert torch.equal(slabs, slabs0), "the slabs depend on whether gsum is given"


def _run_stem(c):
    H, ops = pkg("_hip"), pkg("ops")
    B, Hh, W, Cout = c.shape
    Ho, Wo = R.out_size(Hh, 7, 2, 3), R.out_size(W, 7, 2, 3)
    dt, tdt, st = c.dtype, R.TORCH_DT[c.dtype], H.stream_ptr()
    d, lin, fused, G, gs = R.stem_reference(c.shape, dt)
    img4 = ops.image_to_nhwc4(d["img"].cuda(), dt)
    if c.kind == "stem_fwd":
        w8 = torch.zeros((Cout, 7, 8, 4), dtype=torch.float64)          # tap kw = 7 and channel 3 are zero
        w8[:, :, :7, :3] = d["w"]
        wd, shift = _dev(w8, dt), d["shift"].float().cuda()
        y1, chk1 = R.guarded((B, Ho, Wo, Cout), tdt)
        y2, chk2 = R.guarded((B, Ho, Wo, Cout), tdt)
        with _options(c.opts) as o:
            H.call("dcf_stem7x7_fwd", dt, img4, wd, None, y1, B, Hh, W, Ho, Wo, Cout, 0, st)
            H.call("dcf_stem7x7_fwd", dt, img4, wd, shift, y2, B, Hh, W, Ho, Wo, Cout, 1, st)
        _assert_launches(o.names, "stem_fwd", c.frag + DTN[dt], 2)
        chk1("plain output"); chk2("fused output")
        _assert_bits(y1, lin, dt, "stem plain (n, h, w, c)")
        _assert_bits(y2, fused, dt, "stem fused (n, h, w, c)")
        return
    gy = _dev(d["gy"], dt)
    with _options(c.opts) as o:
        ns = H.call("dcf_conv2d_wgrad_splits", B, Ho, Wo, 32, Cout, 7, 1, 2)
        slabs, chk_s = R.guarded((ns, Cout, 7, 8, 4), torch.float32)
        gsum, chk_g = R.guarded((4 * ns, Cout), torch.float32)
        slabs0, chk_0 = R.guarded((ns, Cout, 7, 8, 4), torch.float32)
        H.call("dcf_stem7x7_wgrad", dt, img4, gy, slabs, gsum, ns, B, Hh, W, Ho, Wo, Cout, st)
        H.call("dcf_stem7x7_wgrad", dt, img4, gy, slabs0, None, ns, B, Hh, W, Ho, Wo, Cout, st)
    _assert_launches(o.names, "stem_wgrad", c.frag + DTN[dt], 2)
    chk_s("slabs"); chk_g("gsum"); chk_0("slabs (gsum null)")
    _assert_sums(slabs, gsum, G, gs, "stem with gsum")
    _assert_sums(slabs0, None, G, gs, "stem gsum null")


def _p(cases):
    return pytest.mark.parametrize("case", cases, ids=[case_id(c) for c in cases])


@_p(IGEMM_CASES)
def test_igemm_exact(case):
    _run_conv(case)


@_p(RS_CASES)
def test_row_sharing_exact(case):
    _run_conv(case)


@_p(LC_CASES)
def test_loader_consumer_exact(case):
    _run_conv(case)


@_p(SP_CASES)
def test_spatial_tile_exact(case):
    _run_conv(case)


@_p(STEM_CASES)
def test_stem_exact(case):
    _run_stem(case)


@_p(WG_GENERIC)
def test_wgrad_generic_exact(case):
    _run_wgrad(case)


@_p(WG3_CASES)
def test_wgrad3_exact(case):
    _run_wgrad(case)


@_p(WG3G_CASES)
def test_wgrad3g_exact(case):
    _run_wgrad(case)


@_p(WGS_CASES)
def test_wgrad_shared_staging_3x3_exact(case):
    _run_wgrad(case)


@_p(WG1_CASES)
def test_wgrad_shared_staging_1x1_stride2_exact(case):
    _run_wgrad(case)


@_p(WGV_CASES)
def test_wgrad_strip_walking_exact(case):
    _run_wgrad(case)
