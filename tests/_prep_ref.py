"""float64 statements of the table-driven parameter kernels -- dcf_weight_prep, dcf_wgrad_finalize(_rows) (csrc/elementwise.hip) and
dcf_weight_prep_fp8 (csrc/conv_fp8.hip) -- the table builder that lays small layers out into their arenas, and the inputs that make a
dropped, doubled or misplaced slab show (test infrastructure; CPU only: imports neither the GPU nor the library).

Every statement reads the arenas the kernel reads (any float dtype; promoted to fp64) through the offsets of one table row and does
everything in fp64.  Next to every sum it returns the number of terms n and the sum of their absolute values A for
_fusion_ref.bound(): a sum of n fp32 terms, in ANY order, lies within (n + 8) * 2^-24 * A of the fp64 value.  The folded-BN factors
(scale = gamma / sqrt(var + eps), invstd) are not sums: a result that carries one gets FACTOR * |want| on top (factor_term()).
tests/test_prep_ref_host.py checks the statements against fp64 autograd through a literal formulation."""
import collections

import numpy as np
import torch

from _fusion_ref import STORE_ULP, assert_within, bound      # noqa: F401  (re-exported: the tests take them from here)

EPS = float(np.float32(1e-5))           # the kernels take eps as a float argument
POISON = 1e30                           # what padded rows / columns and the gaps of the INPUT arenas hold: any read of them shows
CANARY_F = -1234567.0                   # what the fp32 OUTPUT arenas hold before a launch (a fixed odd float, exact in fp32)
CANARY_B = 0xFF                         # ... and the byte arenas
ES = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2}
F8_AMAX_STRIDE = 80                     # DCF_F8_AMAX_STRIDE
# The device forms a folded-BN factor in fp32 as gamma * rsqrtf(var + eps) and multiplies by it once: 0.5 ulp for the add, <= 2 ulp
# for rsqrtf (the public HIP math API table lists 1 ulp), 0.5 ulp for the gamma product (no BN: the factor is exactly 1), 0.5 ulp
# for the final product -- under 4 ulp = 4 * 2^-23 = 8 * 2^-24 relative.
FACTOR = 8.0 * 2.0 ** -24

Layer = collections.namedtuple("Layer", "cout cin taps bn need_dgrad stem nsplit fp8", defaults=(True, True, False, 1, False))


def factor_term(want):
    return FACTOR * want.abs()


def _r4(n):
    return (n + 3) // 4 * 4


def _r256(n):
    return (n + 255) // 256 * 256


def build_table(layers, dtype=torch.float32, gap=4, byte_gap=256):
    """Lays the layers out into the arenas the way backend_hip._layout and the parameter packer do: weight images at 256-byte
    rounded offsets ([wfwd][wdgrad] per layer), [scale cout_pad][shift cout_pad] per layer in ssarena, W [cout][taps][cin] then
    gamma, beta in params, mean, var in buffers, slabs [nsplit][cout_pad][K], gsum [4 * nsplit][cout_pad], w8 [cout_pad][K] bytes,
    wscale [cout_pad].  The rounded sizes are multiples of 256 bytes already at cout_pad >= 32, K >= 32, so the rounding leaves
    no gap: byte_gap unowned bytes follow every weight image, gap unowned elements every other range (both keep the alignment).  A
    layer without need_dgrad gets wdgrad_off = -1 and a RESERVED wd range (rows[i]["wd_reserved"]) nobody may write.

    Returns {"rows": [dict of dcf_conv_param / dcf_f8_param fields per layer], "size": {arena: elements or bytes},
    "own": {arena: [(lo, hi, layer), ...]}} -- own lists what a kernel may write (outputs) or read (inputs)."""
    es = ES[dtype]
    assert gap % 4 == 0 and byte_gap % 256 == 0
    rows = []
    own = {k: [] for k in ("params", "buffers", "grads_w", "warena", "ssarena", "slabs", "gsum", "w8arena", "wsarena")}
    p = b = w = ss = sl = gs = w8 = ws = 0
    for i, L in enumerate(layers):
        assert L.cin % 32 == 0 and L.cout >= 1 and L.nsplit >= 1 and (not L.stem or (L.taps == 7 and L.cin == 32))
        cp, K = (L.cout + 31) // 32 * 32, L.taps * L.cin
        r = dict(cout=L.cout, cin=L.cin, taps=L.taps, cout_pad=cp, nsplit=L.nsplit, flags=1 if L.stem else 0, K=K, bn=bool(L.bn),
                 gamma_off=-1, beta_off=-1, mean_off=-1, var_off=-1, wdgrad_off=-1, wd_reserved=-1, w8_off=-1, wscale_off=-1)
        r["w_off"] = p
        own["params"].append((p, p + L.cout * K, i))
        own["grads_w"].append((p, p + L.cout * K, i))
        p += L.cout * K + gap
        if L.bn:
            for name in ("gamma_off", "beta_off"):
                r[name] = p
                own["params"].append((p, p + L.cout, i))
                p += _r4(L.cout) + gap
            for name in ("mean_off", "var_off"):
                r[name] = b
                own["buffers"].append((b, b + L.cout, i))
                b += _r4(L.cout) + gap
        nbytes = _r256(cp * K * es)
        r["wfwd_off"] = w
        own["warena"].append((w, w + cp * K * es, i))
        w += nbytes + byte_gap
        if L.need_dgrad:
            r["wdgrad_off"] = w
            own["warena"].append((w, w + cp * K * es, i))
        else:
            r["wd_reserved"] = w
        w += nbytes + byte_gap
        r["shift_off"] = ss
        own["ssarena"].append((ss, ss + 2 * cp, i))
        ss += 2 * cp + gap
        r["slab_off"] = sl
        own["slabs"].append((sl, sl + L.nsplit * cp * K, i))
        sl += L.nsplit * cp * K + gap
        r["gsum_off"] = gs
        own["gsum"].append((gs, gs + 4 * L.nsplit * cp, i))
        gs += 4 * L.nsplit * cp + gap
        if L.fp8:
            r["w8_off"], r["wscale_off"] = w8, ws
            own["w8arena"].append((w8, w8 + cp * K, i))
            own["wsarena"].append((ws, ws + cp, i))
            w8 += _r256(cp * K) + byte_gap
            ws += cp + gap
        rows.append(r)
    size = dict(params=p, buffers=max(b, 4), warena=w, ssarena=ss, slabs=sl, gsum=gs, w8arena=max(w8, 256), wsarena=max(ws, 4),
                amax=len(layers) * F8_AMAX_STRIDE)
    return dict(rows=rows, size=size, own=own, es=es, dtype=dtype)


def owned_mask(T, arena, n=None):
    """bool [size]: True where some layer owns the element / byte."""
    m = np.zeros(T["size"]["params" if arena == "grads_w" else arena] if n is None else n, dtype=bool)
    for lo, hi, _ in T["own"][arena]:
        assert not m[lo:hi].any(), "%s: owned ranges overlap at layer %d" % (arena, _)
        m[lo:hi] = True
    return m


CONV_FIELDS = ("w_off", "gamma_off", "beta_off", "mean_off", "var_off", "wfwd_off", "wdgrad_off", "shift_off", "slab_off", "gsum_off",
               "cout", "cin", "taps", "cout_pad", "nsplit", "flags")


def conv_fields(r):
    """The dcf_conv_param fields of a row, in struct order (pad0, pad1 = 0)."""
    return tuple(int(r[k]) for k in CONV_FIELDS) + (0, 0)


# ---------------------------------------------------------------------------------------------------------------- branch selector
def finalize_branch(K, grouped=True):
    """k_wgrad_finalize's selector: ("grouped", G) for short rows, else ("long", [ncol of every kb round])."""
    K4 = K // 4
    G = 1 if (K4 >= 256 or not grouped) else 256 // K4
    if G > 1:
        return "grouped", G
    return "long", [min(4, (K4 - kb + 255) // 256) for kb in range(0, K4, 1024)]


def finalize_unrolls(K, grouped=True):
    """Slab-loop unroll factors a row of K meets, in slabs: 8 * G (grouped), 8 / 4 / 2 for one / two / three-four columns."""
    kind, v = finalize_branch(K, grouped)
    if kind == "grouped":
        return [8 * v]
    return sorted({{1: 8, 2: 4, 3: 2, 4: 2}[c] for c in v})


def prep_items(layers):
    """(conv, tap, 64 x 64 tile) work items of k_weight_prep."""
    return sum(L.taps * (((L.cout + 31) // 32 * 32 + 63) // 64) * ((L.cin + 63) // 64) for L in layers)


def stem_keep(K=224):
    """bool [K] of the stem's [7][8][4] row: False at the structural zeros (tap kw = 7, channel 3)."""
    k = np.arange(K)
    return (((k & 31) >> 2) != 7) & ((k & 3) != 3)


# ---------------------------------------------------------------------------------------------------------------- input makers
def _signed(g, shape, lo, hi):
    """Mixed signs, magnitudes uniform in [lo, hi)."""
    mag = lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)
    sgn = torch.where(torch.rand(shape, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    return (mag * sgn).numpy()


def make_params(T, seed, zero_rows=()):
    """(params, buffers) fp32: W magnitudes in [0.05, 0.3), gamma in [0.5, 1.5), both signs; beta, mean in +-[0.02, 0.2); var in
    [0.5, 1.5).  Everything no layer owns is POISON.  zero_rows: (layer, row) pairs whose W row is all zero."""
    g = torch.Generator().manual_seed(seed)
    params = np.full(T["size"]["params"], POISON, dtype=np.float32)
    buffers = np.full(T["size"]["buffers"], POISON, dtype=np.float32)
    for r in T["rows"]:
        n = r["cout"] * r["K"]
        params[r["w_off"]:r["w_off"] + n] = _signed(g, (n,), 0.05, 0.3)
        if r["bn"]:
            c = r["cout"]
            params[r["gamma_off"]:r["gamma_off"] + c] = _signed(g, (c,), 0.5, 1.5)
            params[r["beta_off"]:r["beta_off"] + c] = _signed(g, (c,), 0.02, 0.2)
            buffers[r["mean_off"]:r["mean_off"] + c] = _signed(g, (c,), 0.02, 0.2)
            buffers[r["var_off"]:r["var_off"] + c] = 0.5 + torch.rand(c, generator=g, dtype=torch.float64).numpy()
    for li, row in zero_rows:
        r = T["rows"][li]
        params[r["w_off"] + row * r["K"]:r["w_off"] + (row + 1) * r["K"]] = 0.0
    return params, buffers


def slab_exponents(n, g):
    """One power of two per slab: exponents spread over [-4, 4] (up to 32 slabs) or [-2, 2], every slab's magnitude its own where the
    range allows.  A slab of magnitude 2^-h among n slabs of at most 2^h is then 2^-2h / n of A while the bound is (n + 8) * 2^-24
    of A: dropping, doubling or misplacing ONE slab moves every element of the row by tens (hundreds of slabs) to thousands of bounds."""
    h = 4 if n <= 32 else 2
    e = torch.arange(n) % (2 * h + 1) - h
    return e[torch.randperm(n, generator=g)].double().numpy()


def make_slabs(T, seed, poison=POISON):
    """(slabs, gsum) fp32.  Slab s of a layer holds mixed-sign values of magnitude [0.5, 1) * 2^e_s (slab_exponents), and so do the
    gsum rows.  Rows co >= cout of every slab, columns co >= cout of every gsum row and the gaps hold `poison`."""
    g = torch.Generator().manual_seed(seed)
    slabs = np.full(T["size"]["slabs"], poison, dtype=np.float32)
    gsum = np.full(T["size"]["gsum"], poison, dtype=np.float32)
    for r in T["rows"]:
        ns, cp, K, c = r["nsplit"], r["cout_pad"], r["K"], r["cout"]
        s = slabs[r["slab_off"]:r["slab_off"] + ns * cp * K].reshape(ns, cp, K)
        s[:, :c] = _signed(g, (ns, c, K), 0.5, 1.0) * 2.0 ** slab_exponents(ns, g)[:, None, None]
        q = gsum[r["gsum_off"]:r["gsum_off"] + 4 * ns * cp].reshape(4 * ns, cp)
        q[:, :c] = _signed(g, (4 * ns, c), 0.5, 1.0) * 2.0 ** slab_exponents(4 * ns, g)[:, None]
    return slabs, gsum


def make_ssarena(T, params, buffers, eps=EPS):
    """ssarena fp32 as a correct dcf_weight_prep leaves it (scale and shift rounded once from fp64; padded channels 0), CANARY_F in
    the gaps -- so that the finalisation tests do not depend on the prep kernel."""
    ss = np.full(T["size"]["ssarena"], CANARY_F, dtype=np.float32)
    for r in T["rows"]:
        scale, shift, _ = _scale_shift(r, params, buffers, eps)
        ss[r["shift_off"]:r["shift_off"] + r["cout_pad"]] = scale
        ss[r["shift_off"] + r["cout_pad"]:r["shift_off"] + 2 * r["cout_pad"]] = shift
    return ss


# ---------------------------------------------------------------------------------------------------------------- statements
def _f64(a, lo, n):
    return np.asarray(a[lo:lo + n], dtype=np.float64)


def _bn(r, params, buffers, eps):
    """(gamma, beta, mean, invstd) fp64 [cout], or None without BN."""
    if not r["bn"]:
        return None
    c = r["cout"]
    return (_f64(params, r["gamma_off"], c), _f64(params, r["beta_off"], c), _f64(buffers, r["mean_off"], c),
            1.0 / np.sqrt(_f64(buffers, r["var_off"], c) + eps))


def _scale_shift(r, params, buffers, eps):
    """scale, shift, A_shift fp64 [cout_pad]: gamma / sqrt(var + eps) (1 without BN), beta - mean * scale (0 without BN) and
    |beta| + |mean * scale|; 0 for co >= cout."""
    cp, c = r["cout_pad"], r["cout"]
    scale, shift, A = np.zeros(cp), np.zeros(cp), np.zeros(cp)
    bn = _bn(r, params, buffers, eps)
    if bn is None:
        scale[:c] = 1.0
    else:
        gamma, beta, mean, inv = bn
        scale[:c] = gamma * inv
        shift[:c] = beta - mean * scale[:c]
        A[:c] = np.abs(beta) + np.abs(mean * scale[:c])
    return scale, shift, A


def _t(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) for a in arrays)


def weight_prep_statement(r, params, buffers, eps=EPS):
    """dict of fp64 tensors: scale, shift, A_shift [cout_pad]; wf [cout_pad][taps][cin] = scale * W with zero rows for co >= cout;
    wd [cin][taps][cout_pad] = the transpose of the same values."""
    cp, c, K = r["cout_pad"], r["cout"], r["K"]
    scale, shift, A = _scale_shift(r, params, buffers, eps)
    wf = np.zeros((cp, r["taps"], r["cin"]))
    wf[:c] = (_f64(params, r["w_off"], c * K).reshape(c, K) * scale[:c, None]).reshape(c, r["taps"], r["cin"])
    out = dict(zip(("scale", "shift", "A_shift", "wf", "wd"), _t(scale, shift, A, wf, wf.transpose(2, 1, 0))))
    return out


def weight_prep_fp8_statement(r, params, buffers, amax_block, eps=EPS):
    """dict of fp64 tensors: bn [cout] (1 without BN); am [cout_pad] = max|W| * |bn|; wscale [cout_pad] = am / 448 (1 for an
    all-zero row, 0 for co >= cout); target [cout_pad][K] = bn * W (0 for co >= cout); amax [F8_AMAX_STRIDE] = the rolled block:
    [64] <- max of [0..63], [0..63] <- 0, the rest as it was."""
    cp, c, K = r["cout_pad"], r["cout"], r["K"]
    bnp = _bn(r, params, buffers, eps)
    bn = np.ones(c) if bnp is None else bnp[0] * bnp[3]
    W = _f64(params, r["w_off"], c * K).reshape(c, K)
    am, wscale, target = np.zeros(cp), np.zeros(cp), np.zeros((cp, K))
    am[:c] = np.abs(W).max(1) * np.abs(bn)
    wscale[:c] = np.where(am[:c] > 0, am[:c] / 448.0, 1.0)
    target[:c] = W * bn[:, None]
    blk = np.asarray(amax_block, dtype=np.float64).copy()
    assert blk.shape == (F8_AMAX_STRIDE,)
    blk[64] = blk[:64].max()
    blk[:64] = 0.0
    return dict(zip(("bn", "am", "wscale", "target", "amax"), _t(bn, am, wscale, target, blk)))


def finalize_statement(r, params, buffers, slabs, gsum, eps=EPS):
    """dict of fp64 tensors for the rows co < cout of one layer:
      G [cout][K] = sum over the slabs (stem: the kw = 7 taps and channel 3 zeroed first), A_G = sum |slab|, n_G = nsplit;
      dW = scale * G (no BN: G), A_dW = |scale| * A_G, n_dW = nsplit;
    and with BN
      dbeta [cout] = sum of the 4 * nsplit gsum rows, A_dbeta, n_dbeta = 4 * nsplit;
      dgamma [cout] = (<W, G> - mean * dbeta) * invstd, A_dgamma = (sum_k |W_k| A_G_k + |mean| A_dbeta) * invstd and
      n_dgamma = max(nsplit + K, 4 * nsplit) + 2: <W, G> is a NESTED sum, so a slab element passes through at most nsplit - 1 adds
      inside G, one product and K - 1 adds of the dot, whatever the order inside either level; a gsum element through 4 * nsplit - 1
      adds and one product; the subtraction is one more for both."""
    ns, cp, K, c = r["nsplit"], r["cout_pad"], r["K"], r["cout"]
    S = _f64(slabs, r["slab_off"], ns * cp * K).reshape(ns, cp, K)[:, :c]
    if r["flags"] & 1:
        S = np.where(stem_keep(K)[None, None, :], S, 0.0)
    G, A_G = S.sum(0), np.abs(S).sum(0)
    bn = _bn(r, params, buffers, eps)
    if bn is None:
        out = dict(zip(("G", "A_G", "dW", "A_dW"), _t(G, A_G, G, A_G)))
        out["n_G"] = out["n_dW"] = ns
        return out
    gamma, beta, mean, inv = bn
    scale = gamma * inv
    W = _f64(params, r["w_off"], c * K).reshape(c, K)
    q = _f64(gsum, r["gsum_off"], 4 * ns * cp).reshape(4 * ns, cp)[:, :c]
    dbeta, A_db = q.sum(0), np.abs(q).sum(0)
    dgamma = ((W * G).sum(1) - mean * dbeta) * inv
    A_dg = ((np.abs(W) * A_G).sum(1) + np.abs(mean) * A_db) * inv
    names = ("G", "A_G", "dW", "A_dW", "dbeta", "A_dbeta", "dgamma", "A_dgamma")
    out = dict(zip(names, _t(G, A_G, scale[:, None] * G, np.abs(scale)[:, None] * A_G, dbeta, A_db, dgamma, A_dg)))
    out["n_G"] = out["n_dW"] = ns
    out["n_dbeta"] = 4 * ns
    out["n_dgamma"] = max(ns + K, 4 * ns) + 2
    return out


# ---------------------------------------------------------------------------------------------------------------- the tests' tables
# Finalisation: cout_pad = 32 throughout, one layer per branch of k_wgrad_finalize; (cout, cin, taps, bn, need_dgrad, stem) and
# the three nsplit assignments -- below the branch's unroll / an exact multiple of it / a multiple plus a tail.
FINALIZE_LAYERS = (
    # K     branch                                   A    B    C
    (Layer(18, 32, 1, True, True, False), (31, 256, 289)),       # 32    G = 32            G-1, 8G, 9G+1 (4 * nsplit > 256 in B, C)
    (Layer(32, 32, 7, True, False, True), (1, 32, 37)),          # 224   G = 4, stem       1, 8G, 9G+1
    (Layer(18, 32, 9, False, True, False), (4, 24, 28)),         # 288   G = 3             G+1, 8G, 9G+1
    (Layer(32, 512, 1, True, True, False), (15, 16, 19)),        # 512   G = 2             8G-1, 8G, 9G+1
    (Layer(32, 64, 9, False, False, False), (7, 8, 17)),         # 576   one column, part  (unroll 8)
    (Layer(32, 1024, 1, True, True, False), (1, 8, 9)),          # 1024  one column, full  (unroll 8)
    (Layer(32, 128, 9, True, False, False), (3, 8, 9)),          # 1152  two columns       (unroll 4)
    (Layer(32, 256, 9, False, True, False), (1, 2, 3)),          # 2304  three of four     (unroll 2)
    (Layer(32, 512, 9, True, True, False), (1, 8, 17)),          # 4608  four + one column (unroll 2, then 8)
)
FINALIZE_CASES = ("below", "multiple", "tail")


def finalize_layers(case):
    i = FINALIZE_CASES.index(case)
    return [L._replace(nsplit=ns[i]) for L, ns in FINALIZE_LAYERS]


def many_1x1_layers(n):
    """n 1x1 cin-32 layers, cout alternating 18 / 32 (irregular first-row prefix sums), every third without BN, nsplit 1..5."""
    return [Layer(18 if i % 2 == 0 else 32, 32, 1, i % 3 != 2, True, False, 1 + i % 5) for i in range(n)]


def prep_layers(n=250):
    """The weight-prep table: cin in {32, 64, 96}, cout in {18, 32, 64, 96}, taps in {1, 7 (stem, cin 32), 9}, every fifth layer
    without BN, every seventh without the dgrad image."""
    out = []
    for i in range(n):
        cin = (32, 64, 96)[i % 3]
        cout = (18, 32, 64, 96)[(i // 3) % 4]
        stem = cin == 32 and i % 4 == 0
        taps = 7 if stem else (1 if i % 5 == 1 else 9)
        out.append(Layer(cout, cin, taps, i % 5 != 0, i % 7 != 3, stem))
    return out


FP8_LAYERS = (
    Layer(32, 64, 1, True, True, False, 1, True),          # K = 64: 16 of the 256 lanes, one trip of the stride loop
    Layer(18, 64, 9, True, True, False, 1, True),          # K = 576: 144 lanes, one trip; cout 18: padded rows
    Layer(32, 128, 9, False, True, False, 1, True),        # K = 1152: 288 vectors, two trips, the last partial; no BN
    Layer(32, 512, 9, True, True, False, 1, True),         # K = 4608: 1152 vectors, five trips, the last partial; all-zero rows
    Layer(32, 64, 1, True, True, False, 1, False),         # not on the fp8 path: w8_off = -1
    Layer(18, 64, 9, False, True, False, 1, True),         # no BN, padded rows, an all-zero row
    Layer(64, 128, 9, True, True, False, 1, True),         # cout_pad 64 = the grid's width
    Layer(64, 64, 1, True, True, False, 1, True),
)
FP8_ZERO_ROWS = ((3, 0), (3, 17), (5, 4))
FP8_AMAX_SLOT = (0, 63, 17, 32, 5, 1, 62, 40)              # where each layer's largest partial maximum is planted


def make_amax(nlayers, seed=0):
    """amax fp32 [nlayers * 80]: [0..63] partial maxima in [0.25, 1) with the layer's maximum 2 + layer at FP8_AMAX_SLOT[layer],
    [64] the previous step's value (100 + layer), [65..79] CANARY_F."""
    g = torch.Generator().manual_seed(900 + seed)
    a = np.full((nlayers, F8_AMAX_STRIDE), CANARY_F, dtype=np.float32)
    a[:, :64] = 0.25 + 0.75 * torch.rand(nlayers, 64, generator=g).numpy()
    for i in range(nlayers):
        a[i, FP8_AMAX_SLOT[i % len(FP8_AMAX_SLOT)]] = 2.0 + i
        a[i, 64] = 100.0 + i
    return a.reshape(-1)


def e4m3_spacing(x):
    """Spacing of the e4m3 grid at |x| <= 448 (fp64 tensor): 2^(e - 3) in the binade [2^e, 2^(e+1)), e >= -6; 2^-9 below."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -6))).clamp(max=8.0)
    return 2.0 ** (e - 3.0)


def assert_allowed(got, want, allowed, what):
    """|got - want| <= allowed element by element (allowed = bound(...) plus whatever non-sum terms the result carries)."""
    got = torch.as_tensor(got).detach().cpu().double().reshape(want.shape)
    assert bool(torch.isfinite(got).all()), "%s: %d non-finite elements" % (what, int((~torch.isfinite(got)).sum()))
    over = (got - want).abs() - allowed.reshape(want.shape)
    worst = int(over.argmax())
    print("%s: max |got - want| %.3g, largest excess over the bound %.3g" % (what, float((got - want).abs().max()), float(over.max())))
    assert float(over.max()) <= 0, "%s: element %d got %.9g want %.9g, %.3g beyond the bound; %d elements beyond it" % (
        what, worst, float(got.reshape(-1)[worst]), float(want.reshape(-1)[worst]), float(over.max()), int((over > 0).sum()))
