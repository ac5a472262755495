"""fp32 statements of the optimiser-step kernels -- k_adam (csrc/elementwise.hip), k_grad_stats / k_amp_update / k_adam_guarded
(csrc/amp.hip), k_adamw_ema_flat / _stride (csrc/optim.hip) -- and the inputs that reach their edges (test infrastructure; CPU only:
imports neither the GPU nor the library).

The library is built with -ffp-contract=off and no fast-math flag, keeps fp32 denormals and uses the IEEE divide and square root, and
numpy's float32 array arithmetic rounds every *, +, -, / and sqrt once and keeps denormals: a restatement that rounds exactly where
include/dcf_hip.h says the kernel rounds is therefore a bit-for-bit specification, not an approximation.  Comparison rule of every
user (same_bits): a NaN equals a NaN, everything else by bits (so -0 is not +0).  tests/test_optim_ref_host.py checks the statements
against fp64 torch.optim.Adam / AdamW, torch._amp_update_scale_ and clip_grad_norm_, so that a wrong statement cannot bless a wrong
kernel (tests/test_gpu_optim_edges.py)."""
import math

import numpy as np

F = np.float32
AMP_PARTS = 1024                        # DCF_AMP_PARTS
THREADS = 256                           # lanes of a workgroup, in every kernel of the family
STRIDE = AMP_PARTS * THREADS            # k_grad_stats' grid stride, in float4s
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
DECAY_MUL = float(F(1.0 - 1e-3 * 0.01))
OMDS = (0.0, 2.0 ** -10, float(F(1e-3)), 1.0)
SIZES_ADAM = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 2043, 2044, 2045, 2047, 2048, 2049, 4099)
# stride shape: 511, 512 and 513 groups with a ragged last group are 2043, 2047 (above) and 2051
SIZES_STRIDE = SIZES_ADAM + (2051,)
SIZES_STATS_N4 = (0, 1, 2, 255, 256, 257, STRIDE - 1, STRIDE, STRIDE + 1, 3 * STRIDE, 3 * STRIDE + 1, 4 * STRIDE - 1, 4 * STRIDE,
                  4 * STRIDE + 1, 7 * STRIDE + 5)
STATS_TAILS = (0, 1, 3)
MASK_KINDS = ("null", "random", "bit63", "bit64", "tail", "ones")


def same_bits(a, b):
    """Per element: both NaN, or the same 32 bits."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def ulps_apart(a, b):
    """Distance of two finite floats of one sign (or zero) in steps of the fp32 grid."""
    a, b = np.array(a, dtype=F).reshape(1), np.array(b, dtype=F).reshape(1)
    return abs(int(a.view(np.int32)[0]) - int(b.view(np.int32)[0]))


# ---------------------------------------------------------------------------------------------------------------- the Adam bodies
def expand_mask(words, n):
    """Per-element bool of the decay mask: bit j % 64 of word j / 64 governs elements 4j .. 4j+3 (a tail group uses its bit like
    any other); None = every element decays."""
    if words is None:
        return np.ones(n, dtype=bool)
    words = np.asarray(words).view(np.uint64).reshape(-1)
    groups = (n + 3) // 4
    j = np.arange(groups, dtype=np.uint64)
    bit = (words[(j >> np.uint64(6)).astype(np.int64)] >> (j & np.uint64(63))) & np.uint64(1)
    return np.repeat(bit != 0, 4)[:n]


def adam_ref(p, g, m, v, lr_over_bc1, inv_sqrt_bc2, gscale, b1, b2, eps, decay_mul=1.0, dec=None, e=None, omd=0.0):
    """One step of the family's shared arithmetic, the header's order, every scalar rounded to fp32 first and every operation on
    float32 arrays:
        gk = g*gscale ;  m' = b1*m + (1-b1)*gk ;  v' = b2*v + ((1-b2)*gk)*gk
        q  = dec ? p*decay_mul : p ;  p' = q - (lr_over_bc1*m') / (sqrt(v')*inv_sqrt_bc2 + eps) ;  e' = e + omd*(p' - e)
    dec: per-element bool (expand_mask), None = every element decays.  Returns (p', m', v', e' or None)."""
    p, g, m, v = (np.asarray(x, dtype=F) for x in (p, g, m, v))
    lr1, isb, gs, b1, b2, eps, dm, omd = (F(x) for x in (lr_over_bc1, inv_sqrt_bc2, gscale, b1, b2, eps, decay_mul, omd))
    one = F(1.0)
    with np.errstate(all="ignore"):
        gk = g * gs
        m1 = b1 * m + (one - b1) * gk
        v1 = b2 * v + ((one - b2) * gk) * gk
        q = p * dm if dec is None else np.where(dec, p * dm, p)
        p1 = q - (lr1 * m1) / (np.sqrt(v1) * isb + eps)
        e1 = None if e is None else np.asarray(e, dtype=F) + omd * (p1 - np.asarray(e, dtype=F))
    assert all(x.dtype == F for x in (p1, m1, v1)) and (e1 is None or e1.dtype == F)
    return p1, m1, v1, e1


def adam_scalars(lr, b1, b2, t):
    """dcf_adam_step's host expressions: doubles formed from the float arguments, 1 - pow(b, t), then (float)(lr / bc1) and
    (float)(1 / sqrt(bc2))."""
    lr, b1, b2 = float(F(lr)), float(F(b1)), float(F(b2))
    bc1, bc2 = 1.0 - math.pow(b1, float(t)), 1.0 - math.pow(b2, float(t))
    return F(lr / bc1), F(1.0 / math.sqrt(bc2))


def bias_is_exactly_one(b, t):
    """b^t < 2^-54: then 1 - b^t is 1.0 in double whatever the last bits of pow are, and the Adam scalars are bitwise."""
    return t * math.log2(float(F(b))) < -54.0


# ---------------------------------------------------------------------------------------------------------------- k_grad_stats
def stats_positions(n):
    """The element indices that name every path of k_grad_stats for n elements: components 0 and 3 of the float4s 0, 1, 255, 256
    (last lane of workgroup 0, first of workgroup 1), stride-1, stride (the last lane's first load, the first lane's second),
    2*stride, 3*stride, 3*stride+1, 4*stride-1 (the third and fourth loads of the unrolled body), 4*stride (its second trip, or the
    remainder loop behind one trip), 5*stride-1 (the remainder loop where lane 0 makes a second trip) and n4-1, where they exist, and
    the n & 3 tail elements."""
    n4 = n >> 2
    quads = sorted(set(i for i in (0, 1, 255, 256, STRIDE - 1, STRIDE, 2 * STRIDE, 3 * STRIDE, 3 * STRIDE + 1, 4 * STRIDE - 1,
                                   4 * STRIDE, 5 * STRIDE - 1, n4 - 1) if 0 <= i < n4))
    return [4 * i + c for i in quads for c in (0, 3)] + [4 * n4 + t for t in range(n & 3)]


def sum_partials(part_sum):
    """k_amp_update's fixed-order double sum of the AMP_PARTS partials: four per lane in order, the xor shuffle tree inside each
    wave of 64, then (w0 + w1) + (w2 + w3)."""
    ps = np.asarray(part_sum, dtype=np.float64).reshape(AMP_PARTS // THREADS, THREADS)
    s = np.zeros(THREADS, dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(ps.shape[0]):
            s = s + ps[k]
        s = s.reshape(THREADS // 64, 64)
        lane = np.arange(64)
        off = 32
        while off > 0:
            s = s + s[:, lane ^ off]
            off >>= 1
        r = s[:, 0]
        return float((r[0] + r[1]) + (r[2] + r[3]))


# ---------------------------------------------------------------------------------------------------------------- k_amp_update
STATE_FIELDS = ("scale_in", "scale_next", "growth_tracker", "found_inf", "applied_steps", "skipped_steps", "grad_norm", "clip_coef",
                "gscale", "lr_over_bc1", "inv_sqrt_bc2")
STATE_FLOATS = ("scale_in", "scale_next", "grad_norm", "clip_coef", "gscale", "lr_over_bc1", "inv_sqrt_bc2")


def amp_update_ref(state, sum_sq, flag, gscale_host, dynamic, growth, backoff, interval, max_norm, lr, b1, b2):
    """k_amp_update's single-lane part from the header's description of dcf_amp_state.  state: dict of STATE_FIELDS as dcf_grad_stats
    left them (scale_in latched); sum_sq: the double sum of the partials; flag: any partial flag.  max_norm None or <= 0 = no
    clipping.  Returns the new dict; the fields the kernel does not write on a skipped step (applied_steps and the three Adam
    scalars) keep their old values."""
    out = dict(state)
    S = F(state["scale_in"])
    max_norm = F(0.0 if max_norm is None else max_norm)
    clip = bool(max_norm > 0)
    with np.errstate(all="ignore"):
        norm = F(math.sqrt(sum_sq) * abs(float(F(gscale_host))) / float(S)) if not math.isnan(sum_sq) else F(np.nan)
        found = bool(flag) or (clip and not np.isfinite(norm))
        coef = F(1.0)
        if clip and not found:
            c = max_norm / (norm + F(1e-6))
            coef = c if c < F(1.0) else F(1.0)
        nxt, tracker = S, int(state["growth_tracker"])
        if found:
            if dynamic:
                nxt, tracker = F(float(S) * float(backoff)), 0
            out["skipped_steps"] = int(state["skipped_steps"]) + 1
        else:
            if dynamic:
                ok = tracker + 1
                if ok == int(interval):
                    grown = F(float(S) * float(growth))
                    if np.isfinite(grown):
                        nxt = grown
                    tracker = 0
                else:
                    tracker = ok
            t = int(state["applied_steps"]) + 1
            out["applied_steps"] = t
            out["lr_over_bc1"], out["inv_sqrt_bc2"] = adam_scalars(lr, b1, b2, t)
            out["gscale"] = (F(gscale_host) / S) * coef
    out["found_inf"] = 1 if found else 0
    out["grad_norm"], out["clip_coef"], out["growth_tracker"], out["scale_next"] = norm, coef, tracker, nxt
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def edge_values():
    """The fixed values planted at known positions of every Adam test vector.  g: +0, -0, a denormal, a value whose square is
    denormal, a large value whose square is finite, +-3e38 (the square overflows; times the step number the gradient itself does),
    inf, NaN.  p: +0, -0, 1e30, and None = the random value stays."""
    with np.errstate(all="ignore"):
        g = np.array([0.0, -0.0, 1e-40, 1e-20, 1e20, 3e38, -3e38, np.inf, np.nan], dtype=F)
    return {"g": g, "g_names": ("+0", "-0", "1e-40", "1e-20", "1e20", "3e38", "-3e38", "inf", "nan"), "p": (0.0, -0.0, 1e30, None)}


N_EDGES = 36                             # every g edge under every p edge


def edge_slots(n):
    """[(element, g edge index, p edge index)]: the 36 pairs at elements 0 .. 35 and, from n = 72, again on the last 36 (the ragged
    tail and the last group); rotated by 5n so that the few elements of a small vector meet other pairs at every size."""
    rot = (5 * n) % N_EDGES
    out = [(j, ((j + rot) % N_EDGES) % 9, ((j + rot) % N_EDGES) // 9) for j in range(min(n, N_EDGES))]
    if n >= 2 * N_EDGES:
        out += [(n - N_EDGES + j, ((j + rot + 7) % N_EDGES) % 9, ((j + rot + 7) % N_EDGES) // 9) for j in range(N_EDGES)]
    return out


def adam_case(n, seed, nonzero_moments, steps=3, edges=True):
    """One test vector: {"p", "m", "v", "e": [n] float32, "g": [steps][n]}.  Uniform [-1, 1) parameters, average and a fresh
    gradient per step; moments zero, or m uniform [-0.5, 0.5) and v uniform [0, 1) with a tenth of v exactly zero; the edge pairs of
    edge_slots planted, the gradient edge multiplied by the step number (3e38 * 2 overflows)."""
    rng = np.random.RandomState(1000 * seed + n % 1000)
    u = lambda lo, hi: rng.uniform(lo, hi, n).astype(F)
    p, e = u(-1, 1), u(-1, 1)
    g = [u(-1, 1) for _ in range(steps)]
    if nonzero_moments:
        m, v = u(-0.5, 0.5), u(0, 1)
        v[rng.uniform(0, 1, n) < 0.1] = 0.0
    else:
        m, v = np.zeros(n, dtype=F), np.zeros(n, dtype=F)
    if edges:
        E = edge_values()
        with np.errstate(all="ignore"):
            for i, gi, pi in edge_slots(n):
                for s in range(steps):
                    g[s][i] = E["g"][gi] * F(s + 1)
                if E["p"][pi] is not None:
                    p[i] = F(E["p"][pi])
    return {"p": p, "m": m, "v": v, "e": e, "g": g}


def mask_words(kind, n, seed=0):
    """The decay masks of the tests as uint64 words (None for "null"): random; only bit 63 (the last of word 0); only bit 64 (the
    first of word 1; no bit at all where there is no second word); only the tail group's bit; all ones, the unused high bits of the
    last word included."""
    groups = (n + 3) // 4
    words = np.zeros((groups + 63) // 64, dtype=np.uint64)
    if kind == "null":
        return None
    if kind == "random":
        bits = np.random.RandomState(77 + seed + n).randint(0, 2, groups)
        for j in np.nonzero(bits)[0]:
            words[j // 64] |= np.uint64(1) << np.uint64(j % 64)
    elif kind == "bit63":
        words[0] = np.uint64(1) << np.uint64(63)
    elif kind == "bit64":
        if len(words) > 1:
            words[1] = np.uint64(1)
    elif kind == "tail":
        words[(groups - 1) // 64] = np.uint64(1) << np.uint64((groups - 1) % 64)
    elif kind == "ones":
        words[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    else:
        raise ValueError(kind)
    return words
