"""GPU: fine-tuning the camera stream -- dcf_image_to_nhwc4_norm and dcf_adamw_ema_step_groups bit for bit
against their host statements (finetune.normalize_image; _finetune_ref.adam_groups_ref = _optim_ref.adam_ref per group), the imported
and normalised camera stream against the torch-CPU restatement, and the trainer with parameter groups: a frozen trunk prefix leaves
the backward plan, its arena ranges keep their bits / exact zeros, and everything else is the step without groups."""
import copy
import os

import numpy as np
import pytest
import torch

import _finetune_ref as FR
import _optim_ref as R
from _paste_util import label_row, make_frame, tiny_crt
from _util import golden_cfg, load_golden, pkg
from _visibility_util import LIM_TINY

pytestmark = pytest.mark.gpu

F = np.float32
LR, B1, B2 = R.LR, R.B1, R.B2
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CANARY = -1234567.0
GUARD = 8


# ---------------------------------------------------------------------------------------------------------------- 1. the norm kernel
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 7), (2, 18, 33), (1, 64, 257)])
def test_image_norm_kernel_is_the_statement_bitwise(shape, dtype):
    """Into a buffer poisoned with NaN: interior, halo and channel 3, every table; the identity equals ops.image_to_nhwc4's bits."""
    ops, FT, Hh_ = pkg("ops"), pkg("finetune"), pkg("_hip")
    B, Hh, W = shape
    img = FR.all_bytes_image(B, Hh, W, seed=Hh)
    if Hh * W >= 256:
        assert all(len(np.unique(img[b, c])) == 256 for b in range(B) for c in range(3))
    dev = torch.from_numpy(img).cuda()
    code = Hh_.dtype_code(dtype)
    for mean, std in FR.NORM_TABLES:
        want = torch.from_numpy(FT.image_to_nhwc4_ref(img, mean, std)).to(TORCH_DT[dtype])          # one rounding to the compute type on store
        y = torch.full((B, Hh + 6, W + 8, 4), float("nan"), dtype=TORCH_DT[dtype], device="cuda")
        ops.image_to_nhwc4_norm(dev, code, mean, std, out=y)
        got = y.cpu()
        assert not torch.isnan(got.float()).any()
        wi = torch.int32 if dtype == "f32" else torch.int16
        assert torch.equal(got.view(wi), want.view(wi)), (shape, dtype, mean)
        assert torch.equal(ops.image_to_nhwc4_norm(dev, code, mean, std).cpu().view(wi), want.view(wi))
    ident = ops.image_to_nhwc4_norm(dev, code, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    plain = ops.image_to_nhwc4(dev, code)
    wi = torch.int32 if dtype == "f32" else torch.int16
    assert torch.equal(ident.view(wi), plain.view(wi))


def test_image_norm_refusals():
    ops, H = pkg("ops"), pkg("_hip")
    dev = torch.zeros((1, 3, 4, 4), dtype=torch.uint8, device="cuda")
    y = torch.zeros((1, 10, 12, 4), device="cuda")
    ok_m, ok_s = H.host_f32([0, 0, 0]), H.host_f32([1, 1, 1])
    for args in ((None, y, ok_m, ok_s), (dev, None, ok_m, ok_s), (dev, y, None, ok_s), (dev, y, ok_m, None)):
        with pytest.raises(H.DcfError):
            H.call("dcf_image_to_nhwc4_norm", H.F32, args[0], args[1], 1, 4, 4, args[2], args[3], H.stream_ptr())
    for mean, std in (([0, float("nan"), 0], [1, 1, 1]), ([float("inf"), 0, 0], [1, 1, 1]), ([0, 0, 0], [1, 0, 1]), ([0, 0, 0], [1, 1, -2]),
                      ([0, 0, 0], [float("inf"), 1, 1]), ([0, 0, 0], [1, float("nan"), 1])):
        with pytest.raises(H.DcfError):
            ops.image_to_nhwc4_norm(dev, H.F32, mean, std)
    with pytest.raises(ValueError):
        ops.image_to_nhwc4_norm(dev, H.F32, [0, 0], [1, 1, 1])
    torch.cuda.synchronize()
    assert not y.any()


# ---------------------------------------------------------------------------------------------------------------- 2. the groups kernel
class Guarded(object):
    """A device array as a 16-byte-aligned view with GUARD canary elements in front and behind."""

    def __init__(self, data, canary=CANARY, dtype=torch.float32):
        n = len(data)
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + n]
        if n:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data)))
        self.edges = self._edges().clone()

    def _edges(self):
        e = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]])
        return e.view(torch.int32) if e.dtype == torch.float32 else e

    def intact(self):
        return torch.equal(self._edges(), self.edges)

    def set(self, data):
        if self.n:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data)))

    def get(self):
        return self.view.cpu().numpy()


def _same(got, want, what):
    ok = R.same_bits(got, want)
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        raise AssertionError("%s: %d of %d elements differ, first at %d: got %r, want %r" % (what, int((~ok).sum()), len(ok), i, got[i], want[i]))


@pytest.fixture(params=["flat", "stride"])
def shape(request):
    H = pkg("_hip")
    H.set_option("ADAMW_SHAPE", request.param)
    yield request.param
    H.set_option("ADAMW_SHAPE", None)


_CLEAN = None


def _clean_state(ops, st, gscale_host, t):
    """The state of applied step t from the real dcf_grad_stats + dcf_amp_update on a clean gradient (scale 1, no clipping)."""
    global _CLEAN
    H = pkg("_hip")
    if _CLEAN is None:
        _CLEAN = Guarded(np.array([3.0, 4.0, 0.0, 0.0, 1.0], dtype=F))
    st.applied_steps.fill_(t - 1)
    ops.grad_stats(_CLEAN.view, st)
    ops.amp_update(st, gscale_host, False, 2.0, 0.5, 2000, None, LR, B1, B2)
    h = H.AmpState.from_buffer_copy(st.raw.cpu().numpy().tobytes())
    assert h.found_inf == 0 and h.applied_steps == t
    return F(h.lr_over_bc1), F(h.inv_sqrt_bc2), F(h.gscale)


WD = 0.01
MUS = (1.0, 0.1, 3.0, 0.0)
# (groups, frozen ids, mask kind, ema_omd or None, guarded, (non-zero moments, gscale, eps))
CONFIGS = [(1, (), "null", None, False, (False, 1.0, 1e-8)), (2, (1,), "random", 2.0 ** -10, False, (True, 0.37, 1e-8)),
           (5, (3,), "tail", None, True, (True, 1.0, 0.0)), (16, (2, 15), "ones", float(F(1e-3)), True, (True, 0.37, 1e-8)),
           (5, (), "bit63", 1.0, False, (False, 1.0, 1e-8)), (2, (0,), "bit64", 0.0, True, (True, 1.0, 1e-8))]
SIZES = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4099, 65539)


def _table(k, frozen, lr):
    rows = [(MUS[g % len(MUS)], g in frozen) for g in range(k)]
    return [(mu, float(F(1.0 - lr * mu * WD)), fz) for mu, fz in rows]


@pytest.mark.parametrize("n", SIZES)
def test_groups_kernel_is_the_statement_bitwise(n, shape):
    """Three steps that carry p, m, v and e, every CONFIGS row: group boundaries inside a wave, on a wave, a workgroup and a chunk
    boundary (_finetune_ref.BOUNDS); a frozen group holds NaN / inf gradients and non-zero moments and keeps all four arrays."""
    ops = pkg("ops")
    dev = torch.device("cuda")
    for ci, (k, frozen, kind, omd, guarded, (nz, gs, eps)) in enumerate(CONFIGS):
        st = ops.AmpState(dev, 1.0) if guarded else None
        ids = FR.segment_ids(n, k)
        el = FR.element_ids(ids, n)
        groups = ops.AdamGroups(ids, k, dev)
        words = R.mask_words(kind, n, ci) if n else None
        Wd = None if words is None else Guarded(words.view(np.int64), 0x5A5A5A5A5A5A5A5A, torch.int64)
        dec = R.expand_mask(words, n)
        c = R.adam_case(n, 40 + ci, nz)
        fz_el = np.isin(el, frozen)
        for s in range(3):                                                # the frozen groups' gradients: NaN and inf, never looked at
            c["g"][s][fz_el] = np.where(np.arange(n)[fz_el] % 2 == 0, np.nan, np.inf).astype(F)
        if fz_el.any():
            assert np.abs(c["m"][fz_el]).sum() > 0 or not nz
        table = _table(k, frozen, LR)
        P, M, V, G = Guarded(c["p"]), Guarded(c["m"]), Guarded(c["v"]), Guarded(c["g"][0])
        E = Guarded(c["e"]) if omd is not None else None
        p, m, v, e = c["p"], c["m"], c["v"], c["e"] if omd is not None else None
        kw = dict(decay_bits=None if Wd is None else Wd.view, ema=None if E is None else E.view, ema_omd=0.0 if omd is None else omd)
        for t in range(1, 4):
            G.set(c["g"][t - 1])
            if guarded:
                lr1, isb, gk = _clean_state(ops, st, gs, t)
                ops.adamw_ema_step_groups(P.view, G.view, M.view, V.view, 123.0, B1, B2, eps, 0, groups, table, 77.0, state=st, **kw)
            else:
                lr1, isb, gk = R.adam_scalars(LR, B1, B2, t) + (gs,)
                ops.adamw_ema_step_groups(P.view, G.view, M.view, V.view, LR, B1, B2, eps, t, groups, table, gs, **kw)
            before = (p, m, v, e)
            p, m, v, e = FR.adam_groups_ref(p, c["g"][t - 1], m, v, e, ids, table, lr1, isb, gk, B1, B2, eps, dec, 0.0 if omd is None else omd)
            what = "n %d %s config %d step %d" % (n, shape, ci, t)
            for got, want, old, name in ((M, m, before[1], "m"), (V, v, before[2], "v"), (P, p, before[0], "p"), (E, e, before[3], "e")):
                if got is not None:
                    _same(got.get(), want, what + " " + name)
                    assert R.same_bits(want[fz_el], old[fz_el]).all()        # (the statement itself keeps the frozen groups)
            assert all(a is None or a.intact() for a in (P, G, M, V, E, Wd)), what
        if guarded:                                                       # found_inf: nothing is stored
            st.found_inf.fill_(1)
            ops.adamw_ema_step_groups(P.view, G.view, M.view, V.view, LR, B1, B2, eps, 0, groups, table, 1.0, state=st, **kw)
            for got, want, name in ((M, m, "m"), (V, v, "v"), (P, p, "p"), (E, e, "e")):
                if got is not None:
                    _same(got.get(), want, "n %d %s config %d skipped %s" % (n, shape, ci, name))


@pytest.mark.parametrize("n", [5, 1025, 2049, 65539])
def test_groups_kernel_with_unit_groups_is_adamw_ema_step(n, shape):
    """mu = 1 everywhere, nothing frozen, every group's decay_mul the single one: the stores of ops.adamw_ema_step on the same inputs,
    plain and guarded, with and without the mask and the average."""
    ops = pkg("ops")
    dev = torch.device("cuda")
    dm = float(F(1.0 - LR * WD))
    for ci, (kind, omd, guarded) in enumerate((("null", None, False), ("random", 2.0 ** -10, False), ("tail", 1.0, True), ("null", None, True))):
        st = ops.AmpState(dev, 1.0) if guarded else None
        groups = ops.AdamGroups(FR.segment_ids(n, 5), 5, dev)
        table = [(1.0, dm, False)] * 5
        words = R.mask_words(kind, n, ci)
        c = R.adam_case(n, 70 + ci, True)
        sides = []
        for side in range(2):
            Wd = None if words is None else Guarded(words.view(np.int64), 0, torch.int64)
            P, M, V, G = Guarded(c["p"]), Guarded(c["m"]), Guarded(c["v"]), Guarded(c["g"][0])
            E = Guarded(c["e"]) if omd is not None else None
            wv, ev, o = None if Wd is None else Wd.view, None if E is None else E.view, 0.0 if omd is None else omd
            for t in range(1, 4):
                G.set(c["g"][t - 1])
                if guarded:
                    _clean_state(ops, st, 0.37, t)
                if side == 0:
                    ops.adamw_ema_step(P.view, G.view, M.view, V.view, LR, B1, B2, 1e-8, 0 if guarded else t, 0.37, dm, wv, ev, o, st)
                else:
                    ops.adamw_ema_step_groups(P.view, G.view, M.view, V.view, LR, B1, B2, 1e-8, 0 if guarded else t, groups, table, 0.37,
                                              decay_bits=wv, ema=ev, ema_omd=o, state=st)
            sides.append([a.get() for a in (P, M, V)] + ([E.get()] if E is not None else []))
        for a, b in zip(*sides):
            _same(b, a, "n %d %s case %d" % (n, shape, ci))


def test_groups_kernel_refusals():
    ops, H = pkg("ops"), pkg("_hip")
    dev = torch.device("cuda")
    n = 64
    buf = torch.zeros(4 * n + 64, device="cuda")
    p, g, m, v = (buf[i * n:(i + 1) * n] for i in range(4))
    ids = np.zeros(n // 4, dtype=np.uint8)
    groups = ops.AdamGroups(ids, 2, dev)
    ok = [(1.0, 1.0, False), (0.1, 1.0, False)]
    ops.adamw_ema_step_groups(p, g, m, v, LR, B1, B2, 1e-8, 1, groups, ok)
    with pytest.raises(ValueError):                                       # an id of at least the group count
        ops.AdamGroups(np.array([0, 2, 1], dtype=np.uint8), 2, dev)
    with pytest.raises(ValueError):                                       # more than 16 groups
        ops.AdamGroups(ids, 17, dev)
    with pytest.raises(ValueError):
        ops.AdamGroups(ids.astype(np.int32), 2, dev)
    with pytest.raises(ValueError):
        ops.adamw_ema_step_groups(p, g, m, v, LR, B1, B2, 1e-8, 1, groups, ok[:1])
    with pytest.raises(ValueError):
        ops.adamw_ema_step_groups(p[:60], g[:60], m[:60], v[:60], LR, B1, B2, 1e-8, 1, ops.AdamGroups(np.zeros(3, dtype=np.uint8), 1, dev), ok[:1])
    for bad in ([(1.0, 1.0, False), (-0.1, 1.0, False)], [(float("nan"), 1.0, False), (1.0, 1.0, False)], [(float("inf"), 1.0, False), (1.0, 1.0, False)],
                [(1.0, float("inf"), False), (1.0, 1.0, False)]):
        with pytest.raises(H.DcfError):
            ops.adamw_ema_step_groups(p, g, m, v, LR, B1, B2, 1e-8, 1, groups, bad)
    tab = (H.AdamGroup * 17)()
    raw = lambda *a: H.call("dcf_adamw_ema_step_groups", *a)
    for ng in (0, 17):                                                    # the C entry's own count check
        with pytest.raises(H.DcfError):
            raw(p, g, m, v, None, None, groups.ids, ng, tab, n, LR, B1, B2, 1e-8, 1, 1.0, 0.0, None, H.stream_ptr())
    with pytest.raises(H.DcfError):                                       # misaligned
        ops.adamw_ema_step_groups(buf[1:n + 1], g, m, v, LR, B1, B2, 1e-8, 1, groups, ok)
    with pytest.raises(H.DcfError):                                       # the average aliases the parameters
        ops.adamw_ema_step_groups(p, g, m, v, LR, B1, B2, 1e-8, 1, groups, ok, ema=p, ema_omd=0.5)
    with pytest.raises(H.DcfError):
        ops.adamw_ema_step_groups(p, g, m, v, LR, B1, B2, 1e-8, 1, groups, ok, ema=buf[4 * n:5 * n], ema_omd=1.5)
    with pytest.raises(H.DcfError):                                       # no step and no state
        ops.adamw_ema_step_groups(p, g, m, v, LR, B1, B2, 1e-8, 0, groups, ok)
    for null in (0, 1, 2, 3):
        args = [p, g, m, v]
        args[null] = None
        with pytest.raises(H.DcfError):
            raw(*(args + [None, None, groups.ids, 2, tab, n, LR, B1, B2, 1e-8, 1, 1.0, 0.0, None, H.stream_ptr()]))
    with pytest.raises(H.DcfError):
        raw(p, g, m, v, None, None, None, 2, tab, n, LR, B1, B2, 1e-8, 1, 1.0, 0.0, None, H.stream_ptr())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 3. the model
def _tiny_cfg(**over):
    cfg = golden_cfg(load_golden("model_tiny.npz"))
    cfg.update(dict(image_height=96, image_width=128, max_num_pc=2048, projection_mode="correct", dtype="f32", loss_reduction="mean",
                    bn_mode="eval", learning_rate=1e-3, batch_size=2, loss_sampling="device", loss_seed=5, deterministic=True))
    cfg["lidar_module"] = dict(cfg["lidar_module"], out_feature2=64, out_feature3=128, out_feature4=192, out_feature5=256)   # deterministic fusion widths
    cfg["fusion"] = dict(enabled=True, K=3, r_max=None, image_channels=64, image_stream="resnet18", zero_init_last=False)
    fusion = over.pop("fusion", None)
    if fusion:
        cfg["fusion"].update(fusion)
    cfg.update(over)
    return cfg


BGR_NORM = {"mean": list(FR.IMAGENET_MEAN[::-1]), "std": list(FR.IMAGENET_STD[::-1])}      # the dataset's planes are B, G, R


def test_imported_and_normalised_camera_stream_against_the_cpu_restatement():
    """A synthesised torchvision trunk imported with `bgr`, image_norm in the dataset's plane order: Plan.forward_image agrees with
    the oracle's image stream on the RGB-ordered, normalised input (the tolerance of the fp32 image-stream parity test)."""
    det = pkg("detfill")
    cfg = _tiny_cfg(deterministic=False, fusion={"image_norm": BGR_NORM})
    net = pkg("model").ObjectDetection_DCF(cfg)
    det.fill_state_dict(net)
    src = FR.tv_state_dict("resnet18", 3)
    net.load_image_trunk(src, "bgr")
    net = net.cuda()
    img = torch.stack([torch.from_numpy(det.synthetic_image(96, 128, 9 + b)) for b in range(2)], 0)
    K = net._ensure_backend(torch.device("cuda", 0))
    K.prepare()
    fmap = net._plan.forward_image(K, img.cuda(), save=False).float().cpu().permute(0, 3, 1, 2)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if k.startswith("image_fpn.")}
    sd.update({FR.PFX + k: v for k, v in src.items() if not k.startswith("fc.")})
    ref = FR.image_stream_norm(sd, img, FR.IMAGENET_MEAN, FR.IMAGENET_STD, "bgr")
    assert fmap.shape == ref.shape
    err = float((fmap - ref).abs().max() / ref.abs().max())
    print("imported + normalised camera stream: max error / max |ref| = %.3g" % err)
    assert err < 1e-3, err
    # the wrong colour order is visible at this tolerance: the check above can fail
    wrong = FR.image_stream_norm(sd, img, FR.IMAGENET_MEAN, FR.IMAGENET_STD, "rgb")
    assert float((fmap - wrong).abs().max() / ref.abs().max()) > 1e-2


# ---------------------------------------------------------------------------------------------------------------- 4. the trainer
SLOTS = [(3.0, -2.5), (8.0, 2.5)]
STEM = ["image_backbone.conv1", "image_backbone.bn1"]
GROUPS_B = [{"match": STEM + ["image_backbone.layer1."], "frozen": True}, {"match": ["image_backbone."], "lr_mult": 0.1}]
GROUPS_C = [{"match": ["image_backbone."], "frozen": True}]
VARIANTS = {"plain": {}, "graphs": {"hip_graphs": True}, "accum": {"grad_accum_steps": 2}, "dynamic": {"loss_scale": "dynamic", "loss_scale_init": 1024.0}}


@pytest.fixture(scope="module")
def world():
    D, FL = pkg("data_import_carla"), pkg("frame_loader")
    cfg = _tiny_cfg()
    frames = [make_frame([label_row(SLOTS[f][0], SLOTS[f][1], -1.0, 0.3)], [30], 1400, LIM_TINY, (96, 128), 70 + f) for f in range(2)]
    host = FL.collate_raw(frames)
    batch = FL.Batch(bboxes=host["bboxes"], num_bboxes=host["num_bboxes"], crt=host["crt"])
    batch["points"] = [p.cuda() for p in host["points"]]
    batch["image"] = torch.stack(host["image"], 0).cuda()
    return {"batch": batch, "geo": D.FrameGeometry(cfg, tiny_crt())}


def _trainer(cfg):
    tr = pkg("train").Train(cfg)
    pkg("detfill").fill_state_dict(tr.model)
    return tr


def _opt_step(tr, world):
    """One optimiser step: one one_step_raw call, or a whole accumulation window of them."""
    k = tr.accum["steps"] if tr.accum is not None else 1
    for _ in range(k):
        tr.one_step_raw(world["geo"], world["batch"])
    torch.cuda.synchronize()


def _state(tr):
    o = tr.optimizer
    return {"g": tr.model.flat_grads.clone(), "p": tr.model.flat_params.detach().clone(), "m": o.m.clone(), "v": o.v.clone()}


def _run(cfg, world, steps=3, profile_step=None):
    tr = _trainer(cfg)
    out = {"tr": tr, "p0": tr.model.flat_params.detach().clone(), "steps": [], "prof": None}
    H = pkg("_hip")
    for s in range(steps):
        if s == profile_step:
            H.call("dcf_prof_reset")
            H.call("dcf_prof_enable", 1)
        try:
            _opt_step(tr, world)
        finally:
            if s == profile_step:
                H.call("dcf_prof_enable", 0)
                out["prof"] = H.prof_read(512)
                H.call("dcf_prof_reset")
        out["steps"].append(_state(tr))
    return out


def _bits(t):
    return t.view(torch.int32)


def _ranges(tr, pred):
    """Arena element mask of the tensors whose key satisfies pred (physical extent, padding to the float4 group included)."""
    mask = torch.zeros(tr.model.flat_params.numel(), dtype=torch.bool)
    for key, shape, off, n, layout in tr.model._table.entries:
        if pred(key):
            mask[off:off + (n + 3) // 4 * 4] = True
    return mask.cuda()


def _launches(prof):
    return sum(int(v[1]) for v in prof.values())


_BASE = {}


def _base(world, variant):
    """Case (a), no groups, per variant: computed once and shared."""
    if variant not in _BASE:
        _BASE[variant] = _run(_tiny_cfg(**VARIANTS[variant]), world, 3, profile_step=1 if variant in ("plain",) else None)
        _BASE[variant]["tr"] = None                                       # only the recorded arenas are kept
    return _BASE[variant]


def _check_frozen(run, frozen, what):
    for s, st in enumerate(run["steps"]):
        assert torch.equal(_bits(st["p"][frozen]), _bits(run["p0"][frozen])), "%s step %d: frozen parameters moved" % (what, s + 1)
        for name in ("m", "v", "g"):
            assert int(_bits(st[name][frozen]).count_nonzero()) == 0, "%s step %d: frozen %s is not exact zeros" % (what, s + 1, name)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_trainer_with_a_frozen_prefix_and_a_slow_group(world, variant):
    """(b) stem + layer1 frozen, the rest of image_backbone. at lr_mult 0.1, against (a) without groups, three optimiser steps."""
    O = pkg("optim")
    a = _base(world, variant)
    cfg = _tiny_cfg(param_groups=copy.deepcopy(GROUPS_B), **VARIANTS[variant])
    b = _run(cfg, world, 3, profile_step=1 if variant == "plain" else None)
    tr = b["tr"]
    assert tr.model._plan.img_frozen == 2 and tr.frozen_range is not None
    frozen = _ranges(tr, lambda k: O.group_of(k, tr.param_groups) == 1)
    slow = _ranges(tr, lambda k: O.group_of(k, tr.param_groups) == 2)
    base = ~(frozen | slow)
    lo, hi = tr.frozen_range
    assert int(frozen.sum()) == hi - lo and bool(frozen[lo:hi].all())      # one contiguous arena range
    _check_frozen(b, frozen, variant)
    a1, b1 = a["steps"][0], b["steps"][0]
    assert torch.equal(_bits(b1["g"][~frozen]), _bits(a1["g"][~frozen])), "gradients outside the frozen range differ from the step without groups"
    assert int(_bits(a1["g"][frozen]).count_nonzero()) > 0                 # (a) does compute them
    assert torch.equal(_bits(b1["p"][base]), _bits(a1["p"][base])), "group-0 parameters differ from the step without groups"
    assert not torch.equal(b1["p"][slow], a1["p"][slow])
    # the slow group: the host statement on (a)'s step-1 gradient
    host_gs = 0.5 if variant == "accum" else 1.0
    gs = F(host_gs) / F(1024.0) if variant == "dynamic" else F(host_gs)
    lr1, isb = R.adam_scalars(cfg["learning_rate"], cfg["beta1"], 0.999, 1)
    sel = slow.cpu().numpy()
    n = int(sel.sum())
    want = R.adam_ref(b["p0"].cpu().numpy()[sel], a1["g"].cpu().numpy()[sel], np.zeros(n, F), np.zeros(n, F), F(lr1) * F(0.1), isb, gs,
                      cfg["beta1"], 0.999, 1e-8)
    assert R.same_bits(b1["p"].cpu().numpy()[sel], want[0]).all() and R.same_bits(b1["m"].cpu().numpy()[sel], want[1]).all()
    assert tr.learning_rates() == [1e-3, 0.0, 1e-3 * 0.1]
    # two trainers are bit-identical
    b2 = _run(cfg, world, 3)
    for s in range(3):
        for name in ("g", "p", "m", "v"):
            assert torch.equal(_bits(b["steps"][s][name]), _bits(b2["steps"][s][name])), (variant, s, name)
    if variant == "plain":
        pa, pb = a["prof"], b["prof"]
        assert any(k.startswith("stem_wgrad") for k in pa) and any(k.startswith("maxpool_bwd") for k in pa)
        assert not [k for k in pb if k.startswith("stem_wgrad") or k.startswith("maxpool_bwd")], sorted(pb)
        assert any(k.startswith("adamw_ema_groups") for k in pb) and not any(k.startswith("adamw_ema_groups") for k in pa)
        print("launches per step: no groups %d, stem + layer1 frozen %d" % (_launches(pa), _launches(pb)))
        assert _launches(pb) < _launches(pa)


def test_trainer_with_the_whole_trunk_frozen(world, monkeypatch):
    """(c): no trunk block runs backward; every image_backbone. element keeps its bits and exact-zero m, v, g."""
    O, E = pkg("optim"), pkg("engine")
    a = _base(world, "plain")
    cfg = _tiny_cfg(param_groups=copy.deepcopy(GROUPS_C))
    seen = []
    orig = E.blocks_backward

    def spy(K, blocks, *args, **kw):
        seen.append(blocks)
        return orig(K, blocks, *args, **kw)
    monkeypatch.setattr(E, "blocks_backward", spy)
    c = _run(cfg, world, 3, profile_step=1)
    tr = c["tr"]
    assert tr.model._plan.img_frozen == 5
    assert not [bl for bl in seen if any(bl is st for st in tr.model._plan.img_stages)], "a trunk block ran backward"
    assert len(seen) == 3 * 5                                             # the LiDAR stages still do
    frozen = _ranges(tr, lambda k: k.startswith("image_backbone."))
    _check_frozen(c, frozen, "whole trunk")
    a1, c1 = a["steps"][0], c["steps"][0]
    assert torch.equal(_bits(c1["g"][~frozen]), _bits(a1["g"][~frozen]))
    assert torch.equal(_bits(c1["p"][~frozen]), _bits(a1["p"][~frozen]))
    pc = c["prof"]
    assert not [k for k in pc if k.startswith("stem_wgrad") or k.startswith("maxpool_bwd")]
    print("launches per step: no groups %d, whole trunk frozen %d" % (_launches(a["prof"]), _launches(pc)))
    assert _launches(pc) < _launches(a["prof"])


def test_trainer_checkpoint_resumes_to_the_same_bits(world, tmp_path):
    cfg = _tiny_cfg(param_groups=copy.deepcopy(GROUPS_B))
    tr = _trainer(cfg)
    _opt_step(tr, world)
    _opt_step(tr, world)
    path = os.path.join(str(tmp_path), "ck.pt")
    tr.save_checkpoint(path)
    _opt_step(tr, world)
    want = _state(tr)
    tr2 = _trainer(cfg)
    tr2.load_checkpoint(path)
    _opt_step(tr2, world)
    got = _state(tr2)
    for name in ("g", "p", "m", "v"):
        assert torch.equal(_bits(got[name]), _bits(want[name])), name


def test_trainer_refusals_and_optimiser_only_freeze(world):
    T = pkg("train")
    with pytest.raises(ValueError):                                       # a frozen BatchNorm that follows batch statistics is not built
        T.Train(_tiny_cfg(param_groups=copy.deepcopy(GROUPS_B), bn_mode="train", deterministic=False))
    with pytest.raises(ValueError):
        T.Train(_tiny_cfg(param_groups=[{"match": ["image_backbone.layer9."], "frozen": True}]))
    with pytest.raises(ValueError):
        T.Train(_tiny_cfg(param_groups=[{"match": ["image_backbone."], "frozen": True, "lr_mult": 0.1}]))
    with pytest.raises(ValueError):
        T.Train(_tiny_cfg(fusion={"image_pretrained": "/nonexistent/trunk.pth"}))
    # anything but the trunk prefix is an optimiser-only freeze: the gradient is computed, the pass ignores it
    tr = _trainer(_tiny_cfg(param_groups=[{"match": ["image_backbone.layer2.", "lidar_backbone.conv3"], "frozen": True}]))
    assert tr.model._plan.img_frozen == 0 and tr.frozen_range is None
    p0 = tr.model.flat_params.detach().clone()
    _opt_step(tr, world)
    O = pkg("optim")
    frozen = _ranges(tr, lambda k: O.group_of(k, tr.param_groups) == 1)
    st = _state(tr)
    assert torch.equal(_bits(st["p"][frozen]), _bits(p0[frozen])) and int(_bits(st["m"][frozen]).count_nonzero()) == 0
    assert int(_bits(st["g"][frozen]).count_nonzero()) > 0
    assert not torch.equal(st["p"][~frozen], p0[~frozen])
    # no groups: the optimiser object of today
    plain = T.Train(_tiny_cfg())
    assert plain.param_groups is None and plain.optimizer.group_ids is None and plain.learning_rates() == [plain.learning_rate()]


def test_ema_with_image_pretrained_starts_from_the_loaded_weights(world, tmp_path):
    O = pkg("optim")
    src = FR.tv_state_dict("resnet18", 5)
    path = os.path.join(str(tmp_path), "trunk.pth")
    torch.save(src, path)
    cfg = _tiny_cfg(ema_decay=0.99, param_groups=copy.deepcopy(GROUPS_B), fusion={"image_pretrained": path, "image_norm": BGR_NORM})
    tr = pkg("train").Train(cfg)
    sd = tr.model.state_dict()
    assert torch.equal(sd["image_backbone.conv1.weight"].cpu(), src["conv1.weight"].flip(1))           # fusion.image_input_order defaults to bgr
    assert torch.equal(sd["image_backbone.layer4.1.bn2.running_var"].cpu(), src["layer4.1.bn2.running_var"])
    ema = tr.ema_params()
    assert torch.equal(_bits(ema), _bits(tr.model.flat_params.detach()))
    esd = tr.ema_state_dict()
    assert torch.equal(esd["image_backbone.layer1.0.conv1.weight"].cpu(), src["layer1.0.conv1.weight"])
    _opt_step(tr, world)
    frozen = _ranges(tr, lambda k: O.group_of(k, tr.param_groups) == 1)
    assert torch.equal(_bits(tr.ema_params()[frozen]), _bits(tr.model.flat_params.detach()[frozen]))   # the average of a frozen tensor keeps its bits
    assert not torch.equal(tr.ema_params()[~frozen], tr.model.flat_params.detach()[~frozen])
    rgb = pkg("train").Train(_tiny_cfg(fusion={"image_pretrained": path, "image_input_order": "rgb"}))
    assert torch.equal(rgb.model.state_dict()["image_backbone.conv1.weight"].cpu(), src["conv1.weight"])


def test_frozen_prefix_under_the_bucket_hook(world):
    """The backend's bucket hook (what a data-parallel run installs): four finalisations in the order the backward completes them,
    never a frozen row; the ranges handed over still tile the whole arena, the frozen range stays exact zeros and every other
    gradient is the one the single finalisation writes."""
    O = pkg("optim")
    cfg = _tiny_cfg(param_groups=copy.deepcopy(GROUPS_B))
    a, b = _trainer(cfg), _trainer(cfg)
    _opt_step(a, world)
    _opt_step(b, world)
    seen = []
    b.model._backend.bucket_hook = seen.extend
    try:
        _opt_step(b, world)
    finally:
        b.model._backend.bucket_hook = None
    _opt_step(a, world)
    sa, sb = _state(a), _state(b)
    for name in ("g", "p", "m", "v"):
        assert torch.equal(_bits(sa[name]), _bits(sb[name])), name
    assert len(seen) >= 4
    pos = 0
    for lo, hi in sorted(seen):
        assert lo == pos and hi > lo, sorted(seen)
        pos = hi
    assert pos == b.model.flat_params.numel()
    frozen = _ranges(b, lambda k: O.group_of(k, b.param_groups) == 1)
    assert int(_bits(sb["g"][frozen]).count_nonzero()) == 0 and int(_bits(sb["g"][~frozen]).count_nonzero()) > 0
