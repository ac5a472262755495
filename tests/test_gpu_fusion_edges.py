"""The continuous-fusion layer's kernels (csrc/fusion.hip, csrc/fusion_det.hip) against the fp64 statements of tests/_fusion_ref.py
at the smallest shapes at which they can still go wrong: the point sampler on and beyond every border, the neighbour gather on
maps with holes, every backward flavour -- pixel runs (pipelined K = 1..5, unpipelined K = 6..8, FUSION_PIPE = 0, long chunks),
by point with and without the workspace, batched, direct rows, one writer per point, deterministic -- against ONE statement
instead of against each other, and the inverse maps integer for integer.

Bound (tests/_fusion_ref.py::bound): an output that is a sum of n fp32 terms with absolute sum A, in any order, must lie within
1.01 * (n + 8) * 2^-24 * A + ulp_store * |want| of the fp64 value; ulp_store is 0 for fp32 results and 2^-8 / 2^-11 where the
result is stored as bf16 / fp16.  A buffer the kernel adds onto is one more term.  The backward inputs are repaired
(repair_relu_margin) until no ReLU argument lies within 1e-4 of zero -- the fp32 argument is within some 1e-6 of the fp64 one --
so the mask is the same on both sides and the comparison has no slack term.  Integer outputs are compared exactly.

fp16 results: the storage term is relative, which holds for normal numbers only; the fp16 cases use inputs whose stored results are zero
or at least 2^-14 (a positive camera map, repaired point rows in the forward too, a positive upstream gradient), asserted per comparison.

Every test asserts its own preconditions (hole census, run lengths, folded taps, zero terms inside the margin)."""
import functools

import numpy as np
import pytest
import torch

import _fusion_ref as R
from _util import pkg

pytestmark = pytest.mark.gpu

AFF = (10.0, 0.0, 10.0, 400.0)
STRIDE, N_MAX, ROWS, N_PTS = 4, 300, 256, 200
SITES = [(24, 40), (23, 37)]                     # 23 x 37: odd width, 851 pixels -- a multiple of no chunk
CAMS = [(24, 32), (1, 5)]
DTYPES = ["f32", "bf16", "f16"]
HAND_MAPS = ("stripes", "one_owner", "boundary_runs", "sparse_ids")
INIT = 0.125                                     # what the accumulated-onto buffers hold on entry


def _tdt(dtype):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]


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


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _cloud(h, w, seed=0):
    """xyz [N_MAX,3]: every row a point over the site's full length and 60 % of its width (a dense part, a border, an empty part)."""
    g = torch.Generator().manual_seed(100 + seed)
    xyz = torch.zeros(N_MAX, 3)
    xyz[:, 0] = torch.rand(N_MAX, generator=g) * (h * STRIDE / AFF[0])
    xyz[:, 1] = torch.rand(N_MAX, generator=g) * (0.6 * w * STRIDE / AFF[2]) - AFF[3] / AFF[2]
    xyz[:, 2] = torch.rand(N_MAX, generator=g) * 2 - 1
    return xyz


def _census(idx):
    """(pixels with 0 neighbours, with 1 .. K-1, with K) of a map."""
    K = idx.shape[0]
    c = (idx >= 0).sum(0).reshape(-1)
    return int((c == 0).sum()), int(((c > 0) & (c < K)).sum()), int((c == K).sum())


@functools.lru_cache(maxsize=None)
def _pick_rmax(h, w, K, n, seed=0):
    """A radius, chosen on the CPU from the cloud's fp64 distances, at which the map has pixels with 0, with 1 .. K-1 and with K
    neighbours (the middle class is empty by definition for K = 1)."""
    xyz = _cloud(h, w, seed)[:n].double()
    X = ((torch.arange(h, dtype=torch.float64) + 0.5) * STRIDE - AFF[1]) / AFF[0]
    Y = ((torch.arange(w, dtype=torch.float64) + 0.5) * STRIDE - AFF[3]) / AFF[2]
    d = ((X[:, None, None] - xyz[None, None, :, 0]) ** 2 + (Y[None, :, None] - xyz[None, None, :, 1]) ** 2).sqrt().reshape(h * w, n)
    best, best_r = -1, None
    for r in torch.quantile(d.sort(1).values[:, min(K, n) - 1], torch.linspace(0.05, 0.95, 19, dtype=torch.float64)).tolist():
        c = (d <= r).sum(1).clamp(max=K)
        score = min(int((c == 0).sum()), int((c == K).sum()), int(((c > 0) & (c < K)).sum()) if K > 1 else 10 ** 9)
        if score > best:
            best, best_r = score, r
    assert best >= 8, "no radius gives the three classes of pixels"
    return best_r


@functools.lru_cache(maxsize=None)
def _map(name, K, h, w, m, seed=0):
    """int32 [K,h,w] on the CPU.  knn / knn_holes: dcf_knn_bev on the first N_PTS points of the cloud, unbounded / with the radius of
    _pick_rmax; the others: the hand-built maps of tests/_fusion_ref.py with ids below m."""
    if name in ("knn", "knn_holes"):
        ops = pkg("ops")
        cnt = torch.tensor([N_PTS], dtype=torch.int32, device="cuda")
        rmax = _pick_rmax(h, w, K, N_PTS, seed) if name == "knn_holes" else None
        idx = ops.knn_bev(_cloud(h, w, seed).cuda(), cnt, K, h, w, STRIDE, AFF, rmax).cpu()
        n0, npart, nfull = _census(idx)
        if name == "knn_holes":
            assert n0 > 0 and nfull > 0 and (npart > 0 or K == 1), (n0, npart, nfull)
        else:
            assert nfull == h * w
        return R.check_map(idx, N_PTS)
    if name == "stripes":
        return R.map_stripes(K, h, w, m)
    if name == "one_owner":
        return R.map_one_owner(K, h, w, m)
    if name == "boundary_runs":
        idx = R.map_boundary_runs(h, w, m, K)
        assert R.run_lengths(idx[0])[:7] == [16, 32, 15, 17, 1, 48, 16] and int((idx[1:] >= 0).sum()) == 0
        return idx
    if name == "sparse_ids":
        return R.map_sparse_ids(K, h, w, m)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _params(Cb, seed=0):
    g = torch.Generator().manual_seed(7 + Cb + 1000 * seed)
    return (torch.rand(Cb, 3, generator=g) - 0.5) * 0.2, (torch.rand(Cb, generator=g) - 0.5) * 0.2


@functools.lru_cache(maxsize=None)
def _point_rows(Cb, dtype, seed=0):
    g = torch.Generator().manual_seed(11 + Cb + 1000 * seed)
    return (torch.rand(N_MAX, Cb, generator=g) - 0.5).to(_tdt(dtype)).float()


# ------------------------------------------------------------------------------------------------------------------ point sampler
@functools.lru_cache(maxsize=None)
def _uv_frames(Hf, Wf):
    """uv of three frames as a slice of a larger tensor: [3, N_MAX + 20, 2] with stride(0) = 2 * (N_MAX + 20) > 2 * N_MAX."""
    big = torch.zeros(5, N_MAX + 20, 2)
    for b in range(5):
        big[b], _ = R.edge_uv(Hf, Wf, N_MAX + 20, seed=5 + b)
    uv = big[1:4]
    folded, centre, four = R.uv_census(uv[0, :37], Hf, Wf)
    assert folded >= 1 and centre >= 1, "the first 37 points (the short count) hold a folded tap and an exact centre"
    for b in range(3):
        folded, centre, four = R.uv_census(uv[b, :N_MAX], Hf, Wf)
        assert folded >= 20 and centre >= Wf
    return big, uv


@functools.lru_cache(maxsize=None)
def _sampler_inputs(Hf, Wf, Cf, dtype):
    g = torch.Generator().manual_seed(31 + Cf)
    tdt = _tdt(dtype)
    # (fp16: a positive map, so that no sampled value cancels into fp16's subnormal range -- see _fusion_ref.assert_within)
    fmap = (torch.rand(3, Hf, Wf, Cf, generator=g) - (0.5 if dtype != "f16" else -0.25)).to(tdt)
    gfp = (torch.rand(3, N_MAX, Cf, generator=g) - 0.5).to(tdt)
    return fmap, gfp


def _check_fp(fp, fmap, uv, count, n_max, tdt, what):
    n = min(count, n_max)
    want, A = R.point_sample_statement(fmap.float(), uv, n)
    assert bool(torch.isfinite(fp.float()).all()), what + ": rows left unwritten"
    if n:
        R.assert_within(fp[:n].float(), want, 4.0, A, tdt, what)
    if n < n_max:
        assert float(fp[n:n_max].float().abs().max()) == 0.0, what + ": rows past the count are not zero"


def _check_gF(gF, gfp, uv, count, n_max, Hf, Wf, init, what):
    n = min(count, n_max)
    want, A, terms = R.point_sample_bwd_statement(gfp.float(), uv, n, Hf, Wf)
    extra = 1.0 if init else 0.0                            # the value the kernel adds onto is one more term
    R.assert_within(gF, want + init, (terms + extra)[:, None].expand_as(want), A + abs(init), torch.float32, what)
    if not init:
        assert float(gF.reshape(Hf * Wf, -1)[terms == 0].abs().max() if bool((terms == 0).any()) else 0.0) == 0.0


@pytest.mark.parametrize("Cf", [4, 36, 64, 256])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Hf,Wf", CAMS)
def test_point_sampler_single_frame_at_its_edges(Hf, Wf, dtype, Cf):
    """dcf_point_sample_fwd / _bwd: counts 0, 37, n_max and n_max + 5 (clamped on the device).  The forward's output starts as NaN and
    must come back whole, zero past the count; the backward adds onto a map of 0.125."""
    ops, H = pkg("ops"), pkg("_hip")
    code, tdt = H.dtype_code(dtype), _tdt(dtype)
    _, uv = _uv_frames(Hf, Wf)
    fmap, gfp = _sampler_inputs(Hf, Wf, Cf, dtype)
    uv_d, fmap_d, gfp_d = uv[0].cuda(), fmap[0].cuda(), gfp[0].cuda()
    for count in (0, 37, N_MAX, N_MAX + 5):
        cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
        out = torch.full((N_MAX, Cf), float("nan"), device="cuda", dtype=tdt)
        fp = ops.point_sample_fwd(code, fmap_d, uv_d, cnt, N_MAX, out=out)
        _check_fp(fp.cpu(), fmap[0], uv[0], count, N_MAX, tdt, "fwd %s Cf %d count %d" % (dtype, Cf, count))
        gF = torch.full((Hf, Wf, Cf), INIT, device="cuda")
        ops.point_sample_bwd(code, gfp_d, uv_d, cnt, N_MAX, gF)
        _check_gF(gF.cpu(), gfp[0], uv[0], count, N_MAX, Hf, Wf, INIT, "bwd %s Cf %d count %d" % (dtype, Cf, count))
    # n_max = 0: nothing is launched, nothing is touched
    cnt = torch.tensor([37], dtype=torch.int32, device="cuda")
    out = torch.full((1, Cf), float("nan"), device="cuda", dtype=tdt)
    ops.point_sample_fwd(code, fmap_d, uv_d, cnt, 0, out=out)
    assert bool(torch.isnan(out.float()).all())
    gF = torch.full((Hf, Wf, Cf), INIT, device="cuda")
    ops.point_sample_bwd(code, gfp_d[:1], uv_d, cnt, 0, gF)
    assert bool((gF == INIT).all())


@pytest.mark.parametrize("Cf", [4, 36, 64, 256])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Hf,Wf", CAMS)
def test_point_sampler_batched_with_strided_uv(Hf, Wf, dtype, Cf):
    """dcf_point_sample_fwd_batch / _bwd_batch, B = 3 with counts n_max + 5, 37 and 0, uv a slice of a larger tensor; for Cf 64 / 256
    also dcf_cam_invert (exact against the numpy statement) + dcf_point_sample_bwd_det, whose map starts as NaN."""
    ops, H = pkg("ops"), pkg("_hip")
    code, tdt = H.dtype_code(dtype), _tdt(dtype)
    big, uv = _uv_frames(Hf, Wf)
    fmap, gfp = _sampler_inputs(Hf, Wf, Cf, dtype)
    uv_d = big.cuda()[1:4]
    assert uv_d.is_contiguous() and uv_d.stride(0) > 2 * N_MAX and uv_d.storage_offset() > 0
    counts = (N_MAX + 5, 37, 0)
    cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    out = torch.full((3, N_MAX, Cf), float("nan"), device="cuda", dtype=tdt)
    fp = ops.point_sample_fwd_batch(code, fmap.cuda(), uv_d, cnt, N_MAX, out).cpu()
    gF = ops.point_sample_bwd_batch(code, gfp.cuda(), uv_d, cnt, N_MAX, torch.full((3, Hf, Wf, Cf), INIT, device="cuda")).cpu()
    for b in range(3):
        _check_fp(fp[b], fmap[b], uv[b], counts[b], N_MAX, tdt, "fwd_batch %s Cf %d frame %d" % (dtype, Cf, b))
        _check_gF(gF[b], gfp[b], uv[b], counts[b], N_MAX, Hf, Wf, INIT, "bwd_batch %s Cf %d frame %d" % (dtype, Cf, b))
    if Cf % 64:
        return
    cam = ops.cam_invert(uv_d, cnt, N_MAX, Hf, Wf)
    ws, we = R.cam_map_statement(uv.numpy(), counts, N_MAX, Hf, Wf)
    assert np.array_equal(cam[0].cpu().numpy(), ws) and np.array_equal(cam[1].cpu().numpy()[:len(we)], we)
    assert int(np.diff(ws).max()) > 64                       # a list longer than a wave
    got = torch.full((3, Hf, Wf, Cf), float("nan"), device="cuda")
    ops.point_sample_bwd_det(code, gfp.cuda(), uv_d, cam, got)
    assert bool(torch.isfinite(got).all())
    for b in range(3):
        _check_gF(got[b].cpu(), gfp[b], uv[b], counts[b], N_MAX, Hf, Wf, 0.0, "bwd_det %s Cf %d frame %d" % (dtype, Cf, b))
    assert float(got[2].abs().max()) == 0.0                  # the frame without points: every row stored as zeros


# ------------------------------------------------------------------------------------------------------------------ gather forward
def _fwd_maps():
    return [("knn", N_PTS), ("knn_holes", N_PTS)] + [(name, N_MAX) for name in HAND_MAPS]


def _fwd_rows(P, xyz, idx, w1d, b1, dtype):
    """fp16: rows repaired as for the backward, so that every ReLU term -- and with it every stored sum -- is zero or above 1e-4."""
    return P if dtype != "f16" else R.repair_relu_margin(P, xyz, idx, STRIDE, AFF, w1d, b1, dtype=torch.float16)


def _check_hsum(hs, c, P, xyz, idx, w1d, b1, tdt, what):
    want, cnt, A = R.gather_fwd_statement(P, xyz, idx, STRIDE, AFF, w1d, b1)
    assert torch.equal(c.cpu().double(), cnt), what + ": cnt"
    hs = hs.cpu().float().reshape(want.shape)
    assert bool(torch.isfinite(hs).all()), what + ": pixels left unwritten"
    R.assert_within(hs, want, cnt[:, None].expand_as(want), A, tdt, what)
    if bool((cnt == 0).any()):
        assert float(hs[cnt == 0].abs().max()) == 0.0, what + ": a pixel without neighbours is not zero"


@pytest.mark.parametrize("Cb", [4, 36, 64, 192, 256])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_forward_on_maps_with_holes(dtype, K, Cb):
    """dcf_fusion_gather_fwd on both sites: KNN maps without and with a radius (pixels with 0, with 1 .. K-1 and with K neighbours,
    asserted) and the four hand-built maps.  hsum and cnt start as NaN; cnt is compared exactly."""
    ops, H = pkg("ops"), pkg("_hip")
    code, tdt = H.dtype_code(dtype), _tdt(dtype)
    P0 = _point_rows(Cb, dtype)
    w1d, b1 = _params(Cb)
    for h, w in SITES:
        xyz = _cloud(h, w)
        for name, m in _fwd_maps():
            idx = _map(name, K, h, w, m)
            P = _fwd_rows(P0, xyz, idx, w1d, b1, dtype)
            out = (torch.full((h, w, Cb), float("nan"), device="cuda", dtype=tdt), torch.full((h * w,), float("nan"), device="cuda"))
            hs, c = ops.fusion_gather_fwd(code, P.to(tdt).cuda(), xyz.cuda(), idx.cuda(), STRIDE, AFF, w1d.reshape(-1).cuda(), b1.cuda(), out=out)
            _check_hsum(hs, c, P, xyz, idx, w1d, b1, tdt, "gather_fwd %s K %d Cb %d %dx%d %s" % (dtype, K, Cb, h, w, name))


@pytest.mark.parametrize("Cb", [4, 64, 256])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w", SITES)
def test_gather_forward_batched_with_short_rows_and_strided_xyz(h, w, dtype, Cb):
    """dcf_fusion_gather_fwd_batch, B = 3 with 200, 1 and 0 points: P with 256 rows (< n_max), xyz a slice of a larger tensor."""
    ops, H = pkg("ops"), pkg("_hip")
    code, tdt = H.dtype_code(dtype), _tdt(dtype)
    K, counts = 3, (N_PTS, 1, 0)
    wide = torch.zeros(5, N_MAX + 12, 3, device="cuda")
    wide[:, :N_MAX] = torch.stack([_cloud(h, w, s) for s in range(5)]).cuda()
    xyz_d = wide[1:4]                                        # [3, 312, 3]: frames 936 floats apart, 312 rows each
    assert xyz_d.is_contiguous() and xyz_d.stride(0) == 3 * (N_MAX + 12)
    cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    idx = torch.stack([ops.knn_bev(xyz_d[b], cnt[b:b + 1], K, h, w, STRIDE, AFF, _pick_rmax(h, w, K, N_PTS, 1)) for b in range(3)])
    census = [_census(idx[b].cpu()) for b in range(3)]
    assert census[0][0] > 0 and census[0][1] > 0 and census[0][2] > 0 and census[1][2] == 0 and census[2][0] == h * w, census
    w1d, b1 = _params(Cb)
    P = torch.stack([_fwd_rows(_point_rows(Cb, dtype, s), _cloud(h, w, s + 1), idx[s].cpu(), w1d, b1, dtype)[:ROWS] for s in range(3)])
    hs = torch.full((3, h, w, Cb), float("nan"), device="cuda", dtype=tdt)
    c = torch.full((3, h * w), float("nan"), device="cuda")
    ops.fusion_gather_fwd_batch(code, P.to(tdt).cuda(), xyz_d, idx, STRIDE, AFF, w1d.reshape(-1).cuda(), b1.cuda(), hs, c)
    for b in range(3):
        R.check_map(idx[b].cpu(), max(counts[b], 1))
        _check_hsum(hs[b], c[b], P[b], _cloud(h, w, b + 1), idx[b].cpu(), w1d, b1, tdt, "gather_fwd_batch %s Cb %d frame %d" % (dtype, Cb, b))


# ------------------------------------------------------------------------------------------------------------------ gather backward
@functools.lru_cache(maxsize=32)
def _bwd_case(h, w, K, Cb, dtype, name, m, seed=0, param_seed=None):
    """Repaired inputs and the statement (sums, term counts, absolute sums) of one backward case: cloud, point rows and gradient of
    `seed`, layer parameters of `param_seed` (the frames of a batch share them)."""
    tdt = _tdt(dtype)
    idx = _map(name, K, h, w, m, seed)
    xyz = _cloud(h, w, seed)
    w1d, b1 = _params(Cb, seed if param_seed is None else param_seed)
    g = torch.Generator().manual_seed(17 + Cb + 1000 * seed)
    # (fp16: a positive gradient, so that no dP row stored as fp16 cancels into the subnormal range)
    ghs = (torch.rand(h, w, Cb, generator=g) - (0.5 if dtype != "f16" else -0.25)).to(tdt).float()
    P = R.repair_relu_margin(_point_rows(Cb, dtype, seed), xyz, idx, STRIDE, AFF, w1d, b1, dtype=tdt)
    assert R.relu_margin_terms(P, xyz, idx, STRIDE, AFF, w1d, b1) == 0
    want, slack, n, A = R.fusion_bwd_statement(P, xyz, idx, STRIDE, AFF, w1d, b1, ghs, terms=True)
    assert all(float(s.abs().max()) == 0.0 for s in slack)
    return dict(idx=idx, xyz=xyz, w1d=w1d, b1=b1, ghs=ghs, P=P, want=want, n=n, A=A, khw=(K, h, w))


def _dev(S, tdt, rows=N_MAX):
    return dict(P=S["P"][:rows].to(tdt).cuda().contiguous(), xyz=S["xyz"].cuda(), idx=S["idx"].cuda(), w1d=S["w1d"].reshape(-1).cuda(), b1=S["b1"].cuda(),
                ghs=S["ghs"].to(tdt).cuda())


def _init_params(Cb):
    return torch.full((Cb * 3,), INIT, device="cuda"), torch.full((Cb,), INIT, device="cuda")


def _check_bwd(gP, gw, gb, cases, store, what, rows=N_MAX):
    """gP against the case's dP (rows beyond `rows` do not exist), gw / gb -- started at INIT -- against the sums over `cases`."""
    S = cases[0]
    if gP is not None:
        R.assert_within(gP.float(), S["want"][0][:rows], S["n"][0][:rows], S["A"][0][:rows], store, what + " dP")
        empty = S["n"][0][:rows].sum(1) == 0
        if bool(empty.any()):
            assert float(gP.float().cpu()[empty].abs().max()) == 0.0, what + ": a row without pairs is not zero"
    for i, got, name in ((1, gw, "dW1d"), (2, gb, "db1")):
        want = sum(c["want"][i] for c in cases) + INIT
        n = sum(c["n"][i] for c in cases) + 1.0
        A = sum(c["A"][i] for c in cases) + INIT
        R.assert_within(got.reshape(want.shape), want, n, A, torch.float32, what + " " + name)


def _pixel_run(code, tdt, S, what):
    ops = pkg("ops")
    D = _dev(S, tdt)
    Cb = S["P"].shape[1]
    gP = torch.zeros(N_MAX, Cb, device="cuda")
    gw, gb = _init_params(Cb)
    ops.fusion_gather_bwd(code, D["P"], D["xyz"], D["idx"], STRIDE, AFF, D["w1d"], D["b1"], D["ghs"], gP, gw, gb)
    _check_bwd(gP, gw, gb, [S], torch.float32, what)


def _bwd_maps():
    return [("knn_holes", N_PTS)] + [(name, N_MAX) for name in HAND_MAPS]


@pytest.mark.parametrize("Cb", [4, 36, 64, 128, 192, 256])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_pixel_run_backward_every_K(K, Cb):
    """dcf_fusion_gather_bwd: K = 1..5 are the five instantiations of the pipelined kernel, K = 6..8 reach the unpipelined one.  fp32 on
    every map of both sites; bf16 and fp16 on the KNN map with holes and on boundary_runs."""
    H = pkg("_hip")
    for dtype in DTYPES:
        code, tdt = H.dtype_code(dtype), _tdt(dtype)
        for h, w in SITES:
            for name, m in _bwd_maps():
                if dtype != "f32" and name not in ("knn_holes", "boundary_runs"):
                    continue
                _pixel_run(code, tdt, _bwd_case(h, w, K, Cb, dtype, name, m), "pixel-run %s K %d Cb %d %dx%d %s" % (dtype, K, Cb, h, w, name))


@pytest.mark.parametrize("Cb", [36, 64, 256])
@pytest.mark.parametrize("option", [("FUSION_PIPE", 0), ("FUSION_THREADS_K", 1)])
def test_pixel_run_backward_unpipelined_route_and_long_chunks(option, Cb, set_opt):
    """K = 3 through the unpipelined kernel (FUSION_PIPE = 0), and with 1024 threads in all (FUSION_THREADS_K = 1): chunks of
    h * w * Cb / 1024 pixels -- 33 to 240 here, lengths that end inside a row and leave a short last chunk."""
    H = pkg("_hip")
    set_opt(*option)
    for dtype in DTYPES:
        code, tdt = H.dtype_code(dtype), _tdt(dtype)
        for h, w in SITES:
            for name, m in _bwd_maps():
                _pixel_run(code, tdt, _bwd_case(h, w, 3, Cb, dtype, name, m), "pixel-run %s=%s %s Cb %d %dx%d %s" % (option + (dtype, Cb, h, w, name)))


def _by_point_flavours(code, tdt, S, what, m):
    """Every single-frame flavour that is driven by the inverse map, on one case."""
    ops, H = pkg("ops"), pkg("_hip")
    K, h, w = S["khw"]
    Cb = S["P"].shape[1]
    D = _dev(S, tdt)
    inv = ops.fusion_invert([D["idx"]], N_MAX)
    args = (STRIDE, AFF, D["w1d"], D["b1"], D["ghs"])
    # fp32 accumulator, float atomics / the slotted workspace
    for ws in (None, ops.fusion_bwd_workspace("cuda", Cb)):
        gP = torch.zeros(N_MAX, Cb, device="cuda")
        gw, gb = _init_params(Cb)
        ops.fusion_gather_bwd_inv(code, D["P"], D["xyz"], inv, N_MAX, 0, (K, h, w), *args, gP, gw, gb, ws=ws)
        _check_bwd(gP, gw, gb, [S], torch.float32, what + (" inv+ws" if ws is not None else " inv"))
        if ws is not None:
            assert float(ws.abs().max()) == 0.0, what + ": workspace not left zero"
    # one writer per point: dP in the compute type, buffer starts as NaN; on fewer rows than n_max where the map allows it
    for rows in ((N_MAX, ROWS) if m <= ROWS else (N_MAX,)):
        Dr = _dev(S, tdt, rows)
        gP = torch.full((rows, Cb), float("nan"), device="cuda", dtype=tdt)
        gw, gb = _init_params(Cb)
        ops.fusion_gather_bwd_pts(code, Dr["P"], D["xyz"], inv, N_MAX, 0, (K, h, w), *args, gP, gw, gb)
        _check_bwd(gP, gw, gb, [S], tdt, what + " pts rows %d" % rows, rows)
    # deterministic: sorted map, workspace full of NaN
    sinv = ops.fusion_invert_sorted([D["idx"]], N_MAX)
    dws = ops.fusion_bwd_det_workspace("cuda", K * h * w, Cb, 1)
    dws.fill_(float("nan"))
    for rows in ((N_MAX, ROWS) if m <= ROWS else (N_MAX,)):
        Dr = _dev(S, tdt, rows)
        gP = torch.full((1, rows, Cb), float("nan"), device="cuda", dtype=tdt)
        gw, gb = _init_params(Cb)
        ops.fusion_gather_bwd_det(code, Dr["P"].unsqueeze(0), D["xyz"].unsqueeze(0), sinv, N_MAX, 0, (K, h, w), *args[:4], D["ghs"].unsqueeze(0), gP, gw, gb, dws)
        _check_bwd(gP[0], gw, gb, [S], tdt, what + " det rows %d" % rows, rows)
    # direct rows: dP in the compute type, zero on entry; both workspaces come back zero
    ws = ops.fusion_bwd_workspace("cuda", Cb)
    xws = ops.fusion_bwd_direct_workspace("cuda", K * h * w, Cb, 1)
    gP = torch.zeros(1, N_MAX, Cb, device="cuda", dtype=tdt)
    gw, gb = _init_params(Cb)
    ops.fusion_gather_bwd_direct_batch(code, D["P"].unsqueeze(0), D["xyz"].unsqueeze(0), inv, N_MAX, 0, (K, h, w), *args[:4], D["ghs"].unsqueeze(0), gP, gw, gb, ws, xws)
    _check_bwd(gP[0], gw, gb, [S], tdt, what + " direct")
    assert float(ws.abs().max()) == 0.0 and float(xws.abs().max()) == 0.0, what + ": direct workspaces not left zero"


BY_POINT_MAPS = [("knn_holes", 3, N_PTS), ("knn_holes", 5, N_PTS), ("stripes", 3, N_MAX), ("stripes", 2, ROWS), ("one_owner", 3, N_MAX), ("one_owner", 1, ROWS),
                 ("boundary_runs", 1, N_MAX), ("boundary_runs", 1, ROWS), ("sparse_ids", 2, N_MAX), ("sparse_ids", 3, ROWS)]


@pytest.mark.parametrize("Cb", [64, 128, 192, 256])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w", SITES)
def test_by_point_backward_flavours_against_the_statement(h, w, dtype, Cb):
    """dcf_fusion_gather_bwd_inv (atomics and workspace), _pts (rows 300 and 256), dcf_fusion_invert_sorted + _det (rows 300 and 256) and
    _direct_batch against the one statement, on the KNN maps with holes and the hand-built maps (ids below 300 and below 256)."""
    H = pkg("_hip")
    code, tdt = H.dtype_code(dtype), _tdt(dtype)
    for name, K, m in BY_POINT_MAPS:
        S = _bwd_case(h, w, K, Cb, dtype, name, m)
        _by_point_flavours(code, tdt, S, "%s K %d Cb %d %dx%d %s(m=%d)" % (dtype, K, Cb, h, w, name, m), N_PTS if name == "knn_holes" else m)


@pytest.mark.parametrize("Cb", [64, 256])
def test_by_point_backward_with_a_capped_grid(Cb, set_opt):
    """FUSION_BWD_BLOCKS = 32.  The launcher never goes below 32 workgroups, and the sites above need fewer, so the cap binds only on a
    map with more than 32 * 16 slices of 16 pairs: K = 5 on 48 x 40 (9600 pairs, 600 slices; with 512 or 256 waves in all a wave walks
    two or three slices).  The sites above run under the option as well."""
    H = pkg("_hip")
    set_opt("FUSION_BWD_BLOCKS", 32)
    for dtype in ("f32", "bf16"):
        code, tdt = H.dtype_code(dtype), _tdt(dtype)
        for (h, w), name, K, m in (((48, 40), "knn_holes", 5, N_PTS), ((48, 40), "stripes", 5, ROWS), ((24, 40), "boundary_runs", 1, ROWS), ((23, 37), "knn_holes", 3, N_PTS)):
            if h == 48:                                          # more workgroups wanted than the cap allows
                assert -(-((K * h * w + 15) // 16) // (8 if Cb == 256 else 16)) > 32
            S = _bwd_case(h, w, K, Cb, dtype, name, m)
            _by_point_flavours(code, tdt, S, "capped %s K %d Cb %d %dx%d %s" % (dtype, K, Cb, h, w, name), N_PTS if name == "knn_holes" else m)


@pytest.mark.parametrize("Cb", [64, 128, 192, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_backward_flavours_against_the_statement(dtype, Cb):
    """dcf_fusion_gather_bwd_inv_batch, _direct_batch and _det with B = 3 on 23 x 37: a KNN map with holes, boundary_runs and one_owner
    side by side (K = 3), P with 256 rows, xyz a slice of a larger tensor; dW1d / db1 are the sums over the frames."""
    ops, H = pkg("ops"), pkg("_hip")
    code, tdt = H.dtype_code(dtype), _tdt(dtype)
    h, w = SITES[1]
    K = 3
    # (the frames share the layer's parameters: every case on the first frame's W1d / b1)
    w1d, b1 = _params(Cb, 1)
    cases = [_bwd_case(h, w, K, Cb, dtype, name, m, seed, 1) for name, m, seed in (("knn_holes", N_PTS, 1), ("boundary_runs", ROWS, 2), ("one_owner", ROWS, 3))]
    wide = torch.zeros(5, N_MAX + 12, 3, device="cuda")
    for b, c in enumerate(cases):
        wide[b + 1, :N_MAX] = c["xyz"].cuda()
    xyz_d = wide[1:4]
    P = torch.stack([c["P"][:ROWS] for c in cases]).to(tdt).cuda()
    ghs = torch.stack([c["ghs"] for c in cases]).to(tdt).cuda()
    maps = [c["idx"].cuda() for c in cases]
    args = (STRIDE, AFF, w1d.reshape(-1).cuda(), b1.cuda(), ghs)
    inv = ops.fusion_invert(maps, N_MAX)
    ws = ops.fusion_bwd_workspace("cuda", Cb)
    what = "batch %s Cb %d" % (dtype, Cb)
    gP = torch.zeros(3, ROWS, Cb, device="cuda")
    gw, gb = _init_params(Cb)
    ops.fusion_gather_bwd_inv_batch(code, P, xyz_d, inv, N_MAX, 0, (K, h, w), *args, gP, gw, gb, ws)
    for b in range(3):
        _check_bwd(gP[b], gw, gb, cases[b:] + cases[:b], torch.float32, what + " inv_batch frame %d" % b, ROWS)
    xws = ops.fusion_bwd_direct_workspace("cuda", K * h * w, Cb, 3)
    gP = torch.zeros(3, ROWS, Cb, device="cuda", dtype=tdt)
    gw, gb = _init_params(Cb)
    ops.fusion_gather_bwd_direct_batch(code, P, xyz_d, inv, N_MAX, 0, (K, h, w), *args, gP, gw, gb, ws, xws)
    for b in range(3):
        _check_bwd(gP[b], gw, gb, cases[b:] + cases[:b], tdt, what + " direct_batch frame %d" % b, ROWS)
    assert float(ws.abs().max()) == 0.0 and float(xws.abs().max()) == 0.0
    sinv = ops.fusion_invert_sorted(maps, N_MAX)
    dws = ops.fusion_bwd_det_workspace("cuda", K * h * w, Cb, 3)
    dws.fill_(float("nan"))
    gP = torch.full((3, ROWS, Cb), float("nan"), device="cuda", dtype=tdt)
    gw, gb = _init_params(Cb)
    ops.fusion_gather_bwd_det(code, P, xyz_d, sinv, N_MAX, 0, (K, h, w), *args, gP, gw, gb, dws)
    for b in range(3):
        _check_bwd(gP[b], gw, gb, cases[b:] + cases[:b], tdt, what + " det frame %d" % b, ROWS)


# ------------------------------------------------------------------------------------------------------------------ inverse maps
@pytest.mark.parametrize("h,w", SITES)
def test_inverse_maps_of_the_hand_built_maps_exact(h, w):
    """dcf_fusion_invert (per-segment sets: the order inside a point's pairs is left to timing) and dcf_fusion_invert_sorted (integer for
    integer) against the numpy statement, all hand-built maps of a K in one call."""
    ops = pkg("ops")
    for K, m in ((1, N_MAX), (3, ROWS), (8, N_MAX)):
        maps = [_map(name, K, h, w, m) for name in HAND_MAPS]
        dev = [t.cuda() for t in maps]
        start_u, ent_u = [t.cpu().numpy() for t in ops.fusion_invert(dev, N_MAX)]
        start_s, ent_s = [t.cpu().numpy() for t in ops.fusion_invert_sorted(dev, N_MAX)]
        assert np.array_equal(start_u, start_s)
        off = 0
        for g, t in enumerate(maps):
            ws, wpx, wpt = R._sorted_pairs(t.numpy(), N_MAX)
            seg = start_s[g * (N_MAX + 1):(g + 1) * (N_MAX + 1)]
            assert np.array_equal(seg - off, ws), (K, HAND_MAPS[g])
            sl = slice(off, off + len(wpx))
            assert np.array_equal(ent_s[0][sl], wpx) and np.array_equal(ent_s[1][sl], wpt), (K, HAND_MAPS[g])
            assert np.array_equal(ent_u[1][sl], wpt), (K, HAND_MAPS[g])
            bounds = np.append(ws, len(wpx))
            for q in np.flatnonzero(np.diff(bounds)):
                a, b = off + bounds[q], off + bounds[q + 1]
                assert np.array_equal(np.sort(ent_u[0][a:b]), wpx[bounds[q]:bounds[q + 1]]), (K, HAND_MAPS[g], int(q))
            off += len(wpx)
