"""The fp64 statements of tests/_fusion_ref.py against fp64 autograd through literal formulations, and the map builders and the
input repair against their own contracts -- so that a wrong statement cannot bless a wrong kernel (tests/test_gpu_fusion_edges.py).
CPU only."""
import numpy as np
import pytest
import torch

import _fusion_ref as R
from oracle import model_ref

AFF = (10.0, 0.0, 10.0, 400.0)


def _close(a, b, what, rtol=1e-12):
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= rtol * scale, "%s: off by %g of %g" % (what, float((a - b).abs().max()), scale)


# ---------------------------------------------------------------------------------------------------------------- gather
def _small_gather_case():
    g = torch.Generator().manual_seed(3)
    K, h, w, stride, rows, Cb = 3, 6, 7, 4, 11, 8
    xyz = torch.zeros(rows, 3)
    xyz[:, 0] = torch.rand(rows, generator=g) * (h * stride / AFF[0])
    xyz[:, 1] = torch.rand(rows, generator=g) * (w * stride / AFF[2]) - AFF[3] / AFF[2]
    xyz[:, 2] = torch.rand(rows, generator=g) * 2 - 1
    idx = torch.stack([torch.randperm(rows, generator=g)[:K] for _ in range(h * w)], 1).reshape(K, h, w)
    idx[2, :, ::2] = -1                                      # pixels with two neighbours,
    idx[1:, 1, 0] = -1                                       # with one,
    idx[:, 5, 6] = -1                                        # and the last pixel of the last row with none
    idx = R.check_map(idx, rows)
    P = torch.rand(rows, Cb, generator=g) - 0.5
    w1d = (torch.rand(Cb, 3, generator=g) - 0.5) * 0.2
    b1 = (torch.rand(Cb, generator=g) - 0.5) * 0.2
    ghs = torch.rand(h, w, Cb, generator=g) - 0.5
    return K, h, w, stride, rows, Cb, xyz, idx, P, w1d, b1, ghs


def _literal_gather(P, xyz, idx, stride, w1d, b1):
    """hsum[p] = sum over the valid slots of relu(P[id] + W1d.(dx, dy, z) + b1), pixel by pixel and slot by slot; the offsets are the
    fp32 values the device forms (csrc/fusion_common.h pixel_centre), promoted to double."""
    K, h, w = idx.shape
    xs, xo, ys, yo = [np.float32(v) for v in AFF]
    rows = []
    for i in range(h):
        for j in range(w):
            X = (np.float32(np.float32(i) + np.float32(0.5)) * np.float32(stride) - xo) / xs
            Y = (np.float32(np.float32(j) + np.float32(0.5)) * np.float32(stride) - yo) / ys
            acc = torch.zeros(P.shape[1], dtype=torch.float64)
            for k in range(K):
                t = int(idx[k, i, j])
                if t < 0:
                    continue
                dx = float(np.float32(xyz[t, 0].item()) - X)
                dy = float(np.float32(xyz[t, 1].item()) - Y)
                dz = float(xyz[t, 2])
                acc = acc + torch.relu(P[t] + w1d[:, 0] * dx + w1d[:, 1] * dy + w1d[:, 2] * dz + b1)
            rows.append(acc)
    return torch.stack(rows)


def test_gather_statements_match_fp64_autograd():
    K, h, w, stride, rows, Cb, xyz, idx, P, w1d, b1, ghs = _small_gather_case()
    cnt_want = (idx >= 0).sum(0).reshape(-1)
    assert set(cnt_want.tolist()) == {0, 1, 2, 3}
    P64, w64, b64 = P.double().requires_grad_(True), w1d.double().requires_grad_(True), b1.double().requires_grad_(True)
    hs = _literal_gather(P64, xyz, idx, stride, w64, b64)
    hsum, cnt, A = R.gather_fwd_statement(P, xyz, idx, stride, AFF, w1d, b1)
    _close(hsum, hs.detach(), "hsum")
    assert torch.equal(cnt, cnt_want.double())
    assert bool((hsum[cnt == 0] == 0).all()) and bool((A[cnt == 0] == 0).all()) and bool((A >= hsum).all())
    (hs * ghs.reshape(h * w, Cb).double()).sum().backward()
    (dP, dW, db), slack, (nP, nW, nb), (aP, aW, ab) = R.fusion_bwd_statement(P, xyz, idx, stride, AFF, w1d, b1, ghs, terms=True)
    _close(dP, P64.grad, "dP")
    _close(dW, w64.grad, "dW1d")
    _close(db, b64.grad, "db1")
    # the old two-tuple form is unchanged, and the term bookkeeping is what it says
    again, slack2 = R.fusion_bwd_statement(P, xyz, idx, stride, AFF, w1d, b1, ghs)
    assert all(torch.equal(a, b) for a, b in zip(again, (dP, dW, db))) and all(torch.equal(a, b) for a, b in zip(slack, slack2))
    assert bool((aP >= dP.abs() - 1e-15).all()) and bool((aW >= dW.abs() - 1e-15).all()) and bool((ab >= db.abs() - 1e-15).all())
    assert float(nP.sum()) == float(nb.sum()) and torch.equal(nW[:, 0], nb) and float(nb.max()) <= float((idx >= 0).sum())
    unused = torch.ones(rows, dtype=torch.bool)
    unused[idx[idx >= 0].long()] = False
    assert bool((nP[unused] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("Hf,Wf", [(24, 32), (1, 5)])
def test_sampler_statements_match_bilinear_sample_autograd(Hf, Wf):
    """oracle/model_ref.bilinear_sample in fp64 on the edge list.  It forms ix = u / 4 - 0.5 in the type of uv; the statement forms it
    in fp32 as make_taps does.  So the oracle is given the fp64 uv whose ix IS the statement's fp32 ix (u = (ix + 0.5) * 4, exact in
    fp64): taps, clamp, weights and sums are then compared to 1e-12, and the fp32 step itself is three numpy fp32 operations."""
    n, Cf = 300, 8
    uv, n_lead = R.edge_uv(Hf, Wf, n)
    folded, centre, four = R.uv_census(uv, Hf, Wf)
    assert folded >= 20 and centre >= Wf and (four >= 50 or Hf == 1)
    g = torch.Generator().manual_seed(9)
    fmap = torch.rand(Hf, Wf, Cf, generator=g) - 0.5
    gfp = torch.rand(n, Cf, generator=g) - 0.5
    u32, v32 = uv[:, 0].numpy(), uv[:, 1].numpy()
    ix = (u32 * np.float32(0.25) - np.float32(0.5)).astype(np.float64)
    iy = (v32 * np.float32(0.25) - np.float32(0.5)).astype(np.float64)
    uv64 = torch.from_numpy(np.stack([(ix + 0.5) * 4.0, (iy + 0.5) * 4.0], 1))
    assert np.array_equal(uv64[:, 0].numpy() * 0.25 - 0.5, ix) and np.array_equal(uv64[:, 1].numpy() * 0.25 - 0.5, iy)
    F64 = fmap.double().permute(2, 0, 1).contiguous().requires_grad_(True)
    ref = model_ref.bilinear_sample(F64, uv64)
    fp, A = R.point_sample_statement(fmap, uv, n)
    _close(fp, ref.detach(), "fp")
    assert bool((A >= fp.abs() - 1e-15).all())
    (ref * gfp.double()).sum().backward()
    gF, Ab, cnt = R.point_sample_bwd_statement(gfp, uv, n, Hf, Wf)
    _close(gF, F64.grad.permute(1, 2, 0).reshape(Hf * Wf, Cf), "gF")
    assert float(cnt.sum()) == 4 * n and bool((Ab >= gF.abs() - 1e-15).all()) and float(cnt.max()) >= 150
    # a shorter count reads only the leading points
    fp37, _ = R.point_sample_statement(fmap, uv, 37)
    assert torch.equal(fp37, fp[:37])
    # the integer taps are those of the map statement
    start, ent = R.cam_map_statement(uv.numpy()[None], [n], n, Hf, Wf)
    assert int(start[-1]) == 4 * n and np.array_equal(np.diff(start), cnt.numpy().astype(np.int64)[:len(start) - 1])


# ---------------------------------------------------------------------------------------------------------------- builders
@pytest.mark.parametrize("h,w", [(24, 40), (23, 37)])
@pytest.mark.parametrize("m", [300, 256])
def test_map_builders_build_maps_the_knn_kernel_could_have_produced(h, w, m):
    for K in (1, 2, 3, 5, 8):
        s = R.map_stripes(K, h, w, m)
        assert all(min(R.run_lengths(s[k])) == 1 and max(R.run_lengths(s[k])) == 1 for k in range(K))
        o = R.map_one_owner(K, h, w, m)
        assert int((o >= 0).sum()) == h * w and R.run_lengths(o[0]) == [h * w] and int(o.max()) == m - 1
        sp = R.map_sparse_ids(K, h, w, m)
        used = set(sp.reshape(-1).tolist())
        assert m - 1 in used and m - 2 not in used and m - 3 not in used and all((m - 1 - t) % 3 == 0 for t in used)
        for t in (s, o, sp):
            assert t.dtype == torch.int32 and t.shape == (K, h, w)
            R.check_map(t, m)
    b = R.map_boundary_runs(h, w, m)
    lens = R.run_lengths(b[0])
    assert lens == R.boundary_run_lengths(h * w) and lens[:7] == [16, 32, 15, 17, 1, 48, 16] and sum(lens) == h * w
    starts = np.concatenate([[0], np.cumsum(lens)])
    for unit in (8, 16):                                     # runs begin on, one before and one after a multiple of the chunk / slice
        assert {0, 1, unit - 1} <= set((starts % unit).tolist())
    # the inverse-map statement on it: sorted by point the pairs are in pixel order
    st, px, pt = R._sorted_pairs(b.numpy(), m)
    assert np.array_equal(np.diff(st)[:len(lens)], lens) and np.array_equal(pt, b.reshape(-1).numpy())


def test_check_map_rejects_invalid_maps():
    ok = torch.tensor([[[0, 1]], [[2, -1]]])
    R.check_map(ok, 3)
    for bad in (torch.tensor([[[0, 3]], [[2, -1]]]), torch.tensor([[[0, -1]], [[2, 1]]]), torch.tensor([[[0, 1]], [[0, -1]]]),
                torch.tensor([[[0, -2]], [[2, -1]]])):
        with pytest.raises(AssertionError):
            R.check_map(bad, 3)


# ---------------------------------------------------------------------------------------------------------------- repair
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("Cb", [64, 128, 256])
def test_repair_leaves_no_term_inside_the_margin_and_touches_only_offenders(Cb, dtype):
    g = torch.Generator().manual_seed(7)
    K, h, w, stride, rows = 3, 24, 40, 4, 300
    xyz = torch.zeros(rows, 3)
    xyz[:, 0] = torch.rand(rows, generator=g) * (h * stride / AFF[0])
    xyz[:, 1] = torch.rand(rows, generator=g) * (w * stride / AFF[2]) - AFF[3] / AFF[2]
    xyz[:, 2] = torch.rand(rows, generator=g) * 2 - 1
    idx = R.map_sparse_ids(K, h, w, rows)
    P = (torch.rand(rows, Cb, generator=g) - 0.5).to(dtype).float()
    w1d = (torch.rand(Cb, 3, generator=g) - 0.5) * 0.2
    b1 = (torch.rand(Cb, generator=g) - 0.5) * 0.2
    before = R.relu_margin_terms(P, xyz, idx, stride, AFF, w1d, b1)
    assert before > 0
    fixed = R.repair_relu_margin(P, xyz, idx, stride, AFF, w1d, b1, dtype=dtype)
    assert R.relu_margin_terms(fixed, xyz, idx, stride, AFF, w1d, b1) == 0
    assert torch.equal(fixed.to(dtype).float(), fixed)                       # representable in the storage type
    # exactly the (id, channel) elements with an offending pair moved: the others' arguments never changed
    safe, valid, d, pre, mag = R._gather_terms(P, xyz, idx, stride, AFF, w1d, b1)
    bad = (pre.abs() <= R.RELU_MARGIN) & valid[:, :, None]
    hit = torch.zeros(rows, Cb)
    hit.index_add_(0, safe.reshape(-1), bad.reshape(-1, Cb).float())
    assert torch.equal(fixed != P, hit > 0)
    assert R.repair_relu_margin(fixed, xyz, idx, stride, AFF, w1d, b1, dtype=dtype).equal(fixed)
