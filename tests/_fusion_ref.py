"""float64 statements of the continuous-fusion layer's kernels (csrc/fusion.hip, csrc/fusion_det.hip) and the inputs that put
them at their edges (test infrastructure; CPU only: imports neither the GPU nor the library).

Every statement forms in fp32 exactly what the device forms in fp32 BEFORE any rounding that matters to a decision -- the bilinear
position ix, iy, its floor and the fractions wx, wy (make_taps), the BEV pixel centre and the offsets dx, dy to it (pixel_centre) --
and does everything after that in fp64.  Next to every sum it returns the number of terms n and the sum of their absolute values A:
a sum of n fp32 terms, in ANY order, lies within (n + 8) * 2^-24 * A of the fp64 value (bound()), the 8 covering the roundings inside
one term.  tests/test_fusion_ref_host.py checks the statements against fp64 autograd through a literal formulation."""
import numpy as np
import torch

STORE_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}     # tests/test_gpu_conv.py::_assert_quantised_close
RELU_MARGIN = 1e-4


def bound(n, A, want, store_dtype=torch.float32):
    """|got - want| allowed for an fp32 sum of n terms with absolute sum A, rounded once to store_dtype."""
    n = torch.as_tensor(n, dtype=torch.float64)
    return 1.01 * (n + 8.0) * 2.0 ** -24 * A + STORE_ULP[store_dtype] * want.abs()


def assert_within(got, want, n, A, store_dtype, what):
    """got within bound() of want, element by element.  Precondition for fp16 results: below 2^-14 fp16 is subnormal and a correctly
    rounded store is off by up to 2^-25 whatever |want|, which the relative storage term does not model -- the fp16 cases are built so
    that every stored value is zero or normal, and that is asserted here."""
    got = got.detach().cpu().double().reshape(want.shape)
    if store_dtype == torch.float16:
        assert bool(((want == 0) | (want.abs() >= 2.0 ** -14)).all()), what + ": an fp16 result in the subnormal range"
    assert bool(torch.isfinite(got).all()), "%s: %d non-finite elements" % (what, int((~torch.isfinite(got)).sum()))
    over = (got - want).abs() - bound(n, A, want, store_dtype).reshape(want.shape)
    worst = int(over.argmax())
    print("%s: max |got - want| %.3g, largest excess over the bound %.3g" % (what, float((got - want).abs().max()), float(over.max())))
    assert float(over.max()) <= 0, "%s: element %d got %.9g want %.9g, %.3g beyond the bound; %d elements beyond it" % (
        what, worst, float(got.reshape(-1)[worst]), float(want.reshape(-1)[worst]), float(over.max()), int((over > 0).sum()))


# ---------------------------------------------------------------------------------------------------------------- bilinear sampling
def _taps(uv, Hf, Wf):
    """make_taps in numpy: fp32 ix, iy, floor, wx, wy; clamped integer taps.  uv [n,2] -> (x0, x1, y0, y1 int64, wx, wy fp32)."""
    uv = np.asarray(uv)
    u, v = uv[:, 0].astype(np.float32), uv[:, 1].astype(np.float32)
    ix = u * np.float32(0.25) - np.float32(0.5)
    iy = v * np.float32(0.25) - np.float32(0.5)
    x0f, y0f = np.floor(ix), np.floor(iy)
    wx, wy = ix - x0f, iy - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.clip(x0 + 1, 0, Wf - 1), np.clip(y0 + 1, 0, Hf - 1)
    x0, y0 = np.clip(x0, 0, Wf - 1), np.clip(y0, 0, Hf - 1)
    assert wx.dtype == np.float32 and wy.dtype == np.float32
    return x0, x1, y0, y1, wx, wy


def taps_statement(uv, Hf, Wf):
    """make_taps' integer taps in numpy (fp32 arithmetic as the device does it): [n,4] pixel indices, tap order (y0,x0) (y0,x1) (y1,x0) (y1,x1)."""
    x0, x1, y0, y1, _, _ = _taps(uv, Hf, Wf)
    return np.stack([y0 * Wf + x0, y0 * Wf + x1, y1 * Wf + x0, y1 * Wf + x1], 1)


def tap_weights(uv, Hf, Wf):
    """([n,4] int64 pixel indices, [n,4] fp64 weights) in taps_statement's order: the fractions are fp32, their products fp64."""
    _, _, _, _, wx, wy = _taps(uv, Hf, Wf)
    wx, wy = torch.from_numpy(wx.astype(np.float64)), torch.from_numpy(wy.astype(np.float64))
    wts = torch.stack([(1 - wy) * (1 - wx), (1 - wy) * wx, wy * (1 - wx), wy * wx], 1)
    return torch.from_numpy(taps_statement(uv, Hf, Wf)), wts


def _uv_np(uv, n):
    return (uv.detach().cpu().numpy() if isinstance(uv, torch.Tensor) else np.asarray(uv))[:n]


def point_sample_statement(fmap, uv, n):
    """fmap [Hf,Wf,Cf], uv [>=n,2] -> fp [n,Cf] fp64 = sum over the four taps of f * w, and A_fp = sum |f * w|."""
    Hf, Wf, Cf = fmap.shape
    pix, wts = tap_weights(_uv_np(uv, n), Hf, Wf)
    f64 = fmap.detach().cpu().double().reshape(Hf * Wf, Cf)
    terms = f64[pix] * wts[:, :, None]                      # [n,4,Cf]
    return terms.sum(1), terms.abs().sum(1)


def point_sample_bwd_statement(gfp, uv, n, Hf, Wf):
    """gfp [>=n,Cf] -> gF [Hf*Wf,Cf] fp64 = sum over (point, tap) of g * w, A = sum |g * w| and the number of terms per pixel
    (taps that the border clamp folds onto one pixel count one each, as the device adds them)."""
    Cf = gfp.shape[1]
    pix, wts = tap_weights(_uv_np(uv, n), Hf, Wf)
    g64 = gfp.detach().cpu().double()[:n]
    gF, A = torch.zeros(Hf * Wf, Cf, dtype=torch.float64), torch.zeros(Hf * Wf, Cf, dtype=torch.float64)
    cnt = torch.zeros(Hf * Wf, dtype=torch.float64)
    for t in range(4):
        term = g64 * wts[:, t, None]
        gF.index_add_(0, pix[:, t], term)
        A.index_add_(0, pix[:, t], term.abs())
        cnt.index_add_(0, pix[:, t], torch.ones(n, dtype=torch.float64))
    return gF, A, cnt


def edge_uv(Hf, Wf, n_total, seed=5):
    """The uv list of the sampler tests: beyond / on every border and on the first and last pixel centres (weights exactly 0
    and 1, two taps folded onto one pixel), every centre of one row, the neighbours of a centre, 150 points in one camera pixel, and a
    uniform fill.  Returns uv [n_total,2] fp32 and the number of leading hand-placed points."""
    g = torch.Generator().manual_seed(seed)
    us = [-3.0, 0.0, 2.0, 4.0 * Wf - 2.0, 4.0 * Wf, 4.0 * Wf + 3.0]
    vs = [-3.0, 0.0, 2.0, 4.0 * Hf - 2.0, 4.0 * Hf, 4.0 * Hf + 3.0]
    pts = [(u, v) for u in us for v in vs]
    row = min(Hf - 1, 2)
    pts += [(4.0 * x + 2.0, 4.0 * row + 2.0) for x in range(Wf)]            # every pixel centre of one row, exactly
    cx, cy = np.float32(4.0 * (Wf // 2) + 2.0), np.float32(4.0 * row + 2.0)
    for a in (np.nextafter(cx, np.float32(-1e9)), np.nextafter(cx, np.float32(1e9))):
        for b in (np.nextafter(cy, np.float32(-1e9)), np.nextafter(cy, np.float32(1e9))):
            pts.append((float(a), float(b)))
    uv = torch.zeros(n_total, 2)
    lead = torch.tensor(pts, dtype=torch.float32)
    n_lead = min(len(pts), n_total)
    uv[:n_lead] = lead[:n_lead]
    n_crowd = max(0, min(150, n_total - n_lead))
    px, py = min(Wf - 2, 3), min(Hf - 1, 1)                                  # camera pixel (py, px) is the first tap of all of them
    uv[n_lead:n_lead + n_crowd, 0] = 4.0 * px + 2.0 + torch.rand(n_crowd, generator=g) * 3.9
    uv[n_lead:n_lead + n_crowd, 1] = 4.0 * py + 2.0 + torch.rand(n_crowd, generator=g) * 3.9
    rest = n_total - n_lead - n_crowd
    uv[n_lead + n_crowd:, 0] = torch.rand(rest, generator=g) * (4 * Wf + 8) - 4
    uv[n_lead + n_crowd:, 1] = torch.rand(rest, generator=g) * (4 * Hf + 8) - 4
    return uv, n_lead


def uv_census(uv, Hf, Wf):
    """(points with two taps on one pixel, points exactly on a pixel centre, points whose four taps are four pixels)."""
    pix = taps_statement(uv.numpy(), Hf, Wf)
    _, wts = tap_weights(uv.numpy(), Hf, Wf)
    folded = int(((pix[:, 0] == pix[:, 1]) | (pix[:, 0] == pix[:, 2])).sum())
    centre = int(((wts == 1.0).any(1) & ((wts == 0.0).sum(1) == 3)).sum())
    four = int((np.array([len(set(r)) for r in pix.tolist()]) == 4).sum())
    return folded, centre, four


def cam_map_statement(uv, cnt, n_max, Hf, Wf):
    """Canonical camera-pixel map of dcf_cam_invert: per frame, the keys point * 4 + tap sorted by (pixel, key)."""
    B = uv.shape[0]
    starts, ents, base = [], [], 0
    for b in range(B):
        n = min(int(cnt[b]), n_max)
        pix = taps_statement(uv[b, :n], Hf, Wf).reshape(-1)
        key = np.arange(n * 4)
        order = np.lexsort((key, pix))
        c = np.bincount(pix, minlength=Hf * Wf + 1)
        starts.append(base + np.concatenate([[0], np.cumsum(c)])[:Hf * Wf + 1])
        ents.append(key[order])
        base += n * 4
    return np.concatenate(starts).astype(np.int32), np.concatenate(ents).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- gather
def _gather_terms(P, xyz, idx, stride, aff, w1d, b1):
    """Per (slot, pixel): ids [K,hw] (clamped to 0 in holes), valid [K,hw], d [K,hw,3] fp64 (dx, dy fp32 differences to the fp32
    pixel centre, as pixel_centre and the kernels form them), pre [K,hw,Cb] fp64, and the absolute sum of pre's five parts."""
    idx = torch.as_tensor(idx)
    K, h, w = idx.shape
    xyz = xyz.detach().cpu().float()
    xs, xo, ys, yo = [np.float32(v) for v in aff[:4]]
    X = ((np.arange(h, dtype=np.float32) + np.float32(0.5)) * np.float32(stride) - xo) / xs          # fp32, as the device forms it
    Y = ((np.arange(w, dtype=np.float32) + np.float32(0.5)) * np.float32(stride) - yo) / ys
    assert X.dtype == np.float32 and Y.dtype == np.float32
    Xp = torch.from_numpy(X).repeat_interleave(w)
    Yp = torch.from_numpy(Y).repeat(h)
    ids = idx.reshape(K, h * w).long()
    valid = ids >= 0
    safe = ids.clamp(min=0)
    d = torch.stack(((xyz[safe, 0] - Xp), (xyz[safe, 1] - Yp), xyz[safe, 2]), -1).double()          # fp32 differences, exact in fp64
    P64 = P.detach().cpu().double()
    w64, b64 = w1d.detach().cpu().double().reshape(-1, 3), b1.detach().cpu().double()
    pre = P64[safe] + d @ w64.t() + b64
    mag = P64[safe].abs() + d.abs() @ w64.abs().t() + b64.abs()
    return safe, valid, d, pre, mag


def gather_fwd_statement(P, xyz, idx, stride, aff, w1d, b1):
    """hsum [h*w,Cb] fp64 = sum over the valid slots of relu(P[id] + W1d.(dx,dy,z) + b1), cnt [h*w] (valid slots per pixel) and
    A = sum over the valid slots of |P| + |w0 dx| + |w1 dy| + |w2 dz| + |b1|."""
    safe, valid, d, pre, mag = _gather_terms(P, xyz, idx, stride, aff, w1d, b1)
    v = valid[:, :, None].double()
    return (torch.relu(pre) * v).sum(0), valid.sum(0).double(), (mag * v).sum(0)


def relu_margin_terms(P, xyz, idx, stride, aff, w1d, b1, margin=RELU_MARGIN):
    """Number of valid (pixel, slot, channel) whose fp64 ReLU argument lies within margin of zero."""
    safe, valid, d, pre, mag = _gather_terms(P, xyz, idx, stride, aff, w1d, b1)
    return int(((pre.abs() <= margin) & valid[:, :, None]).sum())


def repair_relu_margin(P, xyz, idx, stride, aff, w1d, b1, margin=RELU_MARGIN, dtype=torch.float32):
    """P with no valid (pixel, slot, channel) whose fp64 ReLU argument lies within margin of zero: while there is one, 2^-6 is added
    to the offending P[id, c], which is rounded to the storage type again.  The fp32 argument is within some 1e-6 of the fp64 one
    here, so the ReLU mask of the repaired inputs is the same in both and the backward comparison needs no slack."""
    P = P.detach().cpu().to(dtype).float().clone()
    rows, Cb = P.shape
    for _ in range(32):
        safe, valid, d, pre, mag = _gather_terms(P, xyz, idx, stride, aff, w1d, b1)
        bad = (pre.abs() <= margin) & valid[:, :, None]
        if not bool(bad.any()):
            return P
        hit = torch.zeros(rows, Cb, dtype=torch.float64)
        hit.index_add_(0, safe.reshape(-1), bad.reshape(-1, Cb).double())
        P = torch.where(hit > 0, P + 2.0 ** -6, P).to(dtype).float()
    raise AssertionError("repair_relu_margin: terms inside the margin after 32 passes")


def fusion_bwd_statement(P, xyz, idx, stride, aff, w1d, b1, ghs, eps=1e-5, terms=False):
    """dP [rows,Cb], dW1d [Cb,3], db1 [Cb] of  hsum[p] = sum_k relu(P[idx_k] + W1d.(dx,dy,z) + b1)  for upstream gradient
    ghs [h,w,Cb], in fp64 (inputs as given), plus the per-output weight of the terms whose ReLU argument is within eps of 0.
    terms=True: also, per output element, the number of non-zero terms n and A = sum |term| (|g| for dP and db1, |g * d| for dW1d)."""
    K, h, w = idx.shape
    rows, Cb = P.shape
    xs, xo, ys, yo = [np.float32(v) for v in aff[:4]]
    X = ((np.arange(h, dtype=np.float32) + np.float32(0.5)) * np.float32(stride) - xo) / xs          # fp32, as the device forms it
    Y = ((np.arange(w, dtype=np.float32) + np.float32(0.5)) * np.float32(stride) - yo) / ys
    P64, g64 = P.double(), ghs.reshape(h * w, Cb).double()
    w64, b64 = w1d.double(), b1.double()
    Xp = torch.from_numpy(X).repeat_interleave(w)
    Yp = torch.from_numpy(Y).repeat(h)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    dP, sP, nP, aP = z(rows, Cb), z(rows, Cb), z(rows, Cb), z(rows, Cb)
    dW, sW, nW, aW = z(Cb, 3), z(Cb, 3), z(Cb, 3), z(Cb, 3)
    db, sb, nb, ab = z(Cb), z(Cb), z(Cb), z(Cb)
    for k in range(K):
        ids = idx[k].reshape(-1).long()
        valid = ids >= 0
        safe = ids.clamp(min=0)
        d = torch.stack(((xyz[safe, 0] - Xp), (xyz[safe, 1] - Yp), xyz[safe, 2]), 1).double()          # fp32 differences, exact in fp64
        pre = P64[safe] + d @ w64.t() + b64
        m = (pre > 0) & valid[:, None]
        amb = (pre.abs() <= eps) & valid[:, None]
        g = g64 * m
        ga = g64.abs() * amb
        dP.index_add_(0, safe, g)
        sP.index_add_(0, safe, ga)
        dW += g.t() @ d
        sW += ga.t() @ d.abs()
        db += g.sum(0)
        sb += ga.sum(0)
        if terms:
            nz = (g != 0).double()
            nP.index_add_(0, safe, nz)
            aP.index_add_(0, safe, g.abs())
            nW += nz.sum(0)[:, None]
            aW += g.abs().t() @ d.abs()
            nb += nz.sum(0)
            ab += g.abs().sum(0)
    if terms:
        return (dP, dW, db), (sP, sW, sb), (nP, nW, nb), (aP, aW, ab)
    return (dP, dW, db), (sP, sW, sb)


# ---------------------------------------------------------------------------------------------------------------- maps
def _sorted_pairs(idx, n_max):
    """numpy statement of the canonical inverse map of ONE KNN map [K,h,w]: (start [n_max+1], ent_pix, ent_pt)."""
    K, h, w = idx.shape
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    pix = np.broadcast_to(((ii << 16) | jj)[None], (K, h, w)).reshape(-1)
    pt = idx.reshape(-1)
    keep = pt >= 0
    pix, pt = pix[keep], pt[keep]
    order = np.lexsort((pix, pt))                           # by point, then by pixel key
    start = np.concatenate([[0], np.cumsum(np.bincount(pt, minlength=n_max + 1))])[:n_max + 1]
    return start.astype(np.int32), pix[order].astype(np.int32), pt[order].astype(np.int32)


def check_map(idx, rows):
    """What every KNN map satisfies (csrc/geometry.hip) and the inverse-map sort relies on: ids in [-1, rows), the valid ids of a
    pixel pairwise distinct, holes only in trailing slots.  Returns the map as a contiguous int32 tensor."""
    t = torch.as_tensor(idx)
    K = t.shape[0]
    a = t.reshape(K, -1).long()
    assert int(a.min()) >= -1 and int(a.max()) < rows, "ids outside [-1, %d)" % rows
    for k in range(1, K):
        assert not bool(((a[k] >= 0) & (a[k - 1] < 0)).any()), "a hole before a valid slot"
        for j in range(k):
            assert not bool(((a[k] >= 0) & (a[k] == a[j])).any()), "a pixel lists a point twice"
    return t.to(torch.int32).contiguous()


STRIPE_STEP = (0, 17, 27, 37, 47, 57, 67, 77)           # slot k is offset by k * STRIPE_STEP[k]


def map_stripes(K, h, w, m):
    """Slot k of pixel p holds (p + k * stride_k) % m: the id changes at every pixel in every slot -- a flush per pixel, no runs."""
    p = torch.arange(h * w)
    off = [(k * STRIPE_STEP[k]) % m for k in range(K)]
    assert len(set(off)) == K and m > 1
    return check_map(torch.stack([(p + o) % m for o in off]).reshape(K, h, w), m)


def map_one_owner(K, h, w, m):
    """Slot 0 holds the same point (the last row, m - 1) everywhere, the other slots are holes: one run across every chunk and slice."""
    idx = torch.full((K, h, w), -1, dtype=torch.int64)
    idx[0] = m - 1
    return check_map(idx, m)


BOUNDARY_RUNS = (16, 32, 15, 17, 1, 48)


def boundary_run_lengths(hw):
    """Run lengths of map_boundary_runs over hw pixels (the last run is cut at the map's end)."""
    out, left, i = [], hw, 0
    while left > 0:
        out.append(min(BOUNDARY_RUNS[i % len(BOUNDARY_RUNS)], left))
        left -= out[-1]
        i += 1
    return out


def map_boundary_runs(h, w, m, K=1):
    """One valid slot (slots 1 .. K-1 are holes, so the pairs are those of K = 1): consecutive points own 16, 32, 15, 17, 1, 48 pixels in row-major order, repeating.  Sorted by point the pairs are in
    pixel order, so the runs begin and end on, one before and one after the multiples of 8 (the pixel-run kernel's chunk) and of 16
    (the by-point kernels' slice of 16 pairs below 65 k pairs): starts 0, 16, 48, 63, 80, 81, 129, 145, 177, ..."""
    lens = boundary_run_lengths(h * w)
    assert len(lens) <= m
    idx = torch.full((K, h * w), -1, dtype=torch.int64)
    idx[0] = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    return check_map(idx.reshape(K, h, w), m)


def run_lengths(idx_slot):
    """Lengths of the runs of equal ids in one slot [h,w] in row-major order."""
    a = np.asarray(idx_slot).reshape(-1)
    edges = np.flatnonzero(np.diff(a) != 0) + 1
    return np.diff(np.concatenate([[0], edges, [a.size]])).tolist()


def map_sparse_ids(K, h, w, m):
    """Only every third id is used -- m - 1, m - 4, ... -- so the highest row is used and the ids just below the count are not; slot k
    of pixel p holds used[(p // 5 + k) % len(used)]: runs of five pixels."""
    used = torch.arange(m - 1, -1, -3)
    assert K <= len(used)
    p = torch.arange(h * w) // 5
    return check_map(torch.stack([used[(p + k) % len(used)] for k in range(K)]).reshape(K, h, w), m)
