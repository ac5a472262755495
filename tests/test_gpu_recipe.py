"""GPU suite: the training recipe in the trainer (lr_schedule / weight_decay / ema_decay) on the tiny golden
config, batch 1, deterministic: true -- the default config's launches, the schedule against a hand-set rate, decay against one
direct kernel call, the weight average and its exchange context, the guarded skip, checkpoints, captured graphs and host waits."""
import numpy as np
import pytest
import torch

from _util import pkg
from test_gpu_amp import Tiny, _equal3

pytestmark = pytest.mark.gpu

SCHED = dict(kind="step", milestones=[1], gamma=0.5, warmup_steps=1)
RECIPE = dict(lr_schedule=SCHED, weight_decay=0.01, ema_decay=0.9, ema_warmup=True)


def tiny(**over):
    return Tiny("f32", deterministic=True, **over)


def _record_calls(monkeypatch, t, s):
    """Names of the library calls of one_step number s that go through _hip.call."""
    H = pkg("_hip")
    names, real = [], H.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)

    with monkeypatch.context() as mp:
        mp.setattr(H, "call", recording)
        t.step(s)
    return names


def test_default_config_makes_the_same_calls(monkeypatch):
    absent = tiny()
    for k in ("lr_schedule", "weight_decay", "weight_decay_exclude", "ema_decay", "ema_warmup", "ema_eval"):
        assert k not in absent.cfg
    spelled = tiny(lr_schedule=None, weight_decay=0.0, weight_decay_exclude=[], ema_decay=None, ema_warmup=False, ema_eval=True)
    runs = []
    for t in (absent, spelled):
        t.step(0)                                      # first step: lazy set-up
        runs.append(_record_calls(monkeypatch, t, 1))
        assert t.tr.recipe is None and t.tr.ema_params() is None and t.tr.ema_state_dict() is None
        assert t.tr.optimizer.ema is None and t.tr.optimizer.decay_bits is None and not t.tr.optimizer.fused
        assert t.tr.learning_rate() == t.cfg["learning_rate"]
        with pytest.raises(RuntimeError):
            with t.tr.ema_weights():
                pass
    assert runs[0] == runs[1]
    assert runs[0].count("dcf_adam_step") == 1 and "dcf_adamw_ema_step" not in runs[0]
    assert _equal3(absent.state(), spelled.state())
    on = tiny(weight_decay=0.01)
    on.step(0)
    names = _record_calls(monkeypatch, on, 1)
    assert names.count("dcf_adamw_ema_step") == 1 and "dcf_adam_step" not in names
    assert [n for n in names if n != "dcf_adamw_ema_step"] == [n for n in runs[0] if n != "dcf_adam_step"]


def test_schedule_equals_a_rate_set_by_hand():
    O = pkg("optim")
    a, b = tiny(lr_schedule=SCHED), tiny()
    assert not a.tr.optimizer.fused                    # a schedule alone keeps dcf_adam_step: the rate goes in by value
    base = a.cfg["learning_rate"]
    s = O.parse_schedule(SCHED)
    rates = [O.lr_at(s, base, k) for k in range(4)]
    assert rates == [0.0, base, base * 0.5, base * 0.5]
    for k in range(3):
        assert a.tr.learning_rate() == rates[k]
        b.tr.optimizer.lr = rates[k]
        a.step(k)
        b.step(k)
        assert _equal3(a.state(), b.state()), k
    assert a.tr.learning_rate() == rates[3] and a.tr.optimizer.lr == base


def test_decay_touches_the_weights_only_and_equals_one_kernel_call():
    O, ops = pkg("optim"), pkg("ops")
    w = 0.01
    a, b = tiny(weight_decay=w), tiny()
    p0 = b.state()[0]
    assert torch.equal(a.state()[0], p0)
    a.step(0)
    b.step(0)
    assert torch.equal(a.tr.model.flat_grads, b.tr.model.flat_grads)
    sa, sb = a.tr.model.state_dict(), b.tr.model.state_dict()
    seen = set()
    for key, shape, off, n, layout in a.tr.model._table.entries:
        same = torch.equal(sa[key], sb[key])
        assert same if len(shape) == 1 else not same, key
        seen.add(len(shape) == 1)
    assert seen == {True, False}
    model = b.tr.model
    words = O.decay_bits(model._table.entries, model.flat_params.numel())
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    lr = b.cfg["learning_rate"]
    ops.adamw_ema_step(p, model.flat_grads, m, v, lr, b.cfg["beta1"], 0.999, 1e-8, 1, 1.0, 1.0 - lr * w,
                       torch.from_numpy(words.view(np.int64)).cuda())
    assert _equal3(a.state(), (p, m, v))
    # weight_decay_exclude: an excluded weight follows the run without decay
    key = next(k for k, shape, off, n, layout in model._table.entries if len(shape) >= 2)
    c = tiny(weight_decay=w, weight_decay_exclude=[key])
    c.step(0)
    sc = c.tr.model.state_dict()
    assert torch.equal(sc[key], sb[key])
    assert all(torch.equal(sc[k], sa[k]) for k, *_ in model._table.entries if k != key)


def _fold(O, cfg, snaps):
    """The average of the parameter snapshots: e = p0, then e + (p_k - e) * omd_k as three eager fp32 ops per call."""
    r = O.parse_optim_config(cfg)
    e = snaps[0].clone()
    for k, p in enumerate(snaps[1:]):
        d = p - e
        d = d * torch.tensor(1.0 - O.ema_decay_at(r, k), dtype=torch.float32, device="cuda")
        e = e + d
    return e


def test_ema_fold_and_the_exchange_context():
    O = pkg("optim")
    t = tiny(ema_decay=0.9, ema_warmup=True)
    snaps = [t.state()[0]]
    assert torch.equal(t.tr.ema_params(), snaps[0])            # before the first step the average is the (filled) parameters
    for k in range(3):
        t.step(k)
        snaps.append(t.state()[0])
    want = _fold(O, t.cfg, snaps)
    ema = t.tr.ema_params()
    assert torch.equal(ema, want)
    assert not torch.equal(want, snaps[-1]) and not torch.equal(want, snaps[0])
    sd, esd = t.tr.model.state_dict(), t.tr.ema_state_dict()
    assert list(sd.keys()) == list(esd.keys())
    from_arena = {k: pkg("engine").ParamTable.view(want, shape, off, n, layout) for k, shape, off, n, layout in t.tr.model._table.entries}
    assert all(torch.equal(esd[k], from_arena[k]) if k in from_arena else torch.equal(esd[k], sd[k]) for k in sd)
    model = t.tr.model
    ptr, eptr, params = model.flat_params.data_ptr(), ema.data_ptr(), snaps[-1]
    _, cls_out, reg_out = t.tr.get_loss_value(t.x, t.img, t.boxes, t.nb)
    cls_out, reg_out = cls_out.clone(), reg_out.clone()
    with t.tr.ema_weights():
        assert torch.equal(model.flat_params, want) and model.flat_params.data_ptr() == ptr
        assert torch.equal(t.tr.optimizer.ema, params) and t.tr.optimizer.ema.data_ptr() == eptr
        _, cls_in, reg_in = t.tr.get_loss_value(t.x, t.img, t.boxes, t.nb)
        assert not torch.equal(cls_in, cls_out) and not torch.equal(reg_in, reg_out)
        with pytest.raises(RuntimeError):
            with t.tr.ema_weights():
                pass
        with pytest.raises(RuntimeError):
            t.tr.one_step(t.x, t.img, t.boxes, t.nb)
        assert torch.equal(model.flat_params, want)            # the refused calls changed nothing
    assert torch.equal(model.flat_params, params) and torch.equal(t.tr.ema_params(), want)
    _, cls_back, _ = t.tr.get_loss_value(t.x, t.img, t.boxes, t.nb)
    assert torch.equal(cls_back, cls_out)                       # the weight images were folded again from the restored arena
    with pytest.raises(KeyError):
        with t.tr.ema_weights():
            raise KeyError("body")
    assert torch.equal(model.flat_params, params) and torch.equal(t.tr.ema_params(), want)
    assert model.flat_params.data_ptr() == ptr and t.tr.ema_params().data_ptr() == eptr
    t.step(3)                                                   # training goes on after the context
    assert torch.equal(t.tr.ema_params(), _fold(O, t.cfg, snaps + [t.state()[0]]))


def test_guarded_skip_leaves_parameters_and_average_and_advances_the_clock():
    t = tiny(loss_scale="dynamic", weight_decay=0.01, ema_decay=0.9, lr_schedule=dict(kind="constant", warmup_steps=8, warmup_start_factor=0.5))
    t.step(0)
    before, ema0 = t.state(), t.tr.ema_params().clone()
    assert not torch.equal(ema0, before[0])
    lr1 = t.tr.learning_rate()
    t.step(1, "nan")
    assert not bool(torch.isfinite(t.tr.model.flat_grads).all()), "the bad frame did not reach the gradient"
    assert _equal3(t.state(), before) and torch.equal(t.tr.ema_params(), ema0)
    a = t.amp()
    assert a["found"] == 1 and a["skipped"] == 1 and a["applied"] == 1
    base = t.cfg["learning_rate"]
    assert lr1 == base * (0.5 + 0.5 * 1 / 8) and t.tr.learning_rate() == base * (0.5 + 0.5 * 2 / 8)
    assert t.tr.optimizer.opt_calls == 2
    t.step(2)
    assert t.amp()["applied"] == 2 and not torch.equal(t.tr.ema_params(), ema0)
    assert bool(torch.isfinite(t.state()[0]).all()) and bool(torch.isfinite(t.tr.ema_params()).all())


def test_checkpoint_carries_the_clock_and_the_average(tmp_path):
    over = dict(lr_schedule=dict(kind="cosine", warmup_steps=1, warmup_start_factor=0.5, total_steps=6), weight_decay=0.01, ema_decay=0.9)
    a = tiny(**over)
    a.step(0)
    a.step(1)
    a.tr.save_checkpoint(str(tmp_path / "ck.pt"), epoch=2)
    a.step(2)
    a.step(3)
    b = tiny(**over)
    assert b.tr.load_checkpoint(str(tmp_path / "ck.pt")) == 2
    assert b.tr.optimizer.opt_calls == 2
    b.step(2)
    b.step(3)
    assert _equal3(a.state(), b.state()) and torch.equal(a.tr.ema_params(), b.tr.ema_params())
    assert a.tr.learning_rate() == b.tr.learning_rate() != a.cfg["learning_rate"]
    # a checkpoint without the new keys (here: the optimiser state as it was written before the recipe existed)
    c = tiny()
    c.step(0)
    c.step(1)
    c.tr.save_checkpoint(str(tmp_path / "plain.pt"))
    ck = torch.load(str(tmp_path / "plain.pt"), map_location="cpu")
    assert "ema" not in ck["optimizer"]
    del ck["optimizer"]["opt_calls"]
    torch.save(ck, str(tmp_path / "old.pt"))
    d = tiny(**over)
    d.tr.load_checkpoint(str(tmp_path / "old.pt"))
    assert d.tr.optimizer.opt_calls == d.tr.optimizer.step_count == 2
    assert torch.equal(d.tr.model.flat_params, c.tr.model.flat_params) and torch.equal(d.tr.ema_params(), c.tr.model.flat_params)
    d.step(2)
    assert not torch.equal(d.tr.ema_params(), d.tr.model.flat_params)


def test_hip_graphs_batch1_matches_eager():
    """Captured graphs with the whole recipe on: three steps within the bounds of test_batch1_hip_graphs_skip_and_match_eager
    (rtol 1e-5, atol 1e-6) of the eager run, the average included."""
    runs = {}
    for graphs in (True, False):
        t = tiny(hip_graphs=graphs, **RECIPE)
        assert t.tr.model.graphs_wanted(1) == graphs
        out = []
        for s in range(3):
            t.step(s)
            out.append((t.tr.model.flat_grads.clone(),) + t.state() + (t.tr.ema_params().clone(),))
        runs[graphs] = out
    for s in range(3):
        for a, b in zip(runs[True][s], runs[False][s]):
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), s
    assert not torch.equal(runs[False][2][4], runs[False][2][1])


def test_no_new_host_synchronisation(monkeypatch):
    """Three one_step calls with schedule + decay + average make exactly as many host-synchronising calls as with none."""
    counts = {}

    def counting(name, fn):
        def wrapped(*a, **k):
            counts[name] = counts.get(name, 0) + 1
            return fn(*a, **k)
        return wrapped

    runs = {}
    for mode, over in (("none", {}), ("recipe", RECIPE)):
        t = tiny(**over)
        t.step(0)                                   # first step: lazy set-up on both paths, not counted
        counts.clear()
        with monkeypatch.context() as mp:
            for owner, name in ((torch.Tensor, "item"), (torch.Tensor, "cpu"), (torch.Tensor, "tolist"), (torch.cuda, "synchronize"),
                                (torch.cuda.Event, "synchronize"), (torch.cuda.Stream, "synchronize")):
                mp.setattr(owner, name, counting(owner.__name__ + "." + name, getattr(owner, name)))
            for s in range(1, 4):
                np.random.seed(100 + s)
                t.tr.one_step(t.x, t.img, t.boxes, t.nb)
                t.tr.learning_rate()
                t.tr.ema_params()
        runs[mode] = dict(counts)
        torch.cuda.synchronize()
    print(runs)
    assert runs["recipe"] == runs["none"]
