"""GPU suite: gradient accumulation (grad_accum_steps / grad_accum_reduce; csrc/optim.hip dcf_grad_accumulate) --
the kernel on every alignment, off means off, the window as an exact left fold, finish_window, the large batch it stands for, the
guarded skip of a whole window, the recipe's clocks, checkpoints inside a window, captured graphs and one collective per window.
Tiny golden config, f32, batch 1, deterministic: true unless stated; the two micro-steps of a window use the two golden frames."""
import numpy as np
import pytest
import torch

from _util import load_golden, pkg
from test_gpu_amp import Tiny, _equal3, tiny_cfg, tiny_input
from test_gpu_recipe import SCHED, _fold, _record_calls

pytestmark = pytest.mark.gpu


class Acc(Tiny):
    """Tiny("f32", deterministic=True) with both golden frames at hand: micro(frame, s, bad) = one one_step on that frame alone with
    np.random.seed(100 + s), bad = "nan" written into one voxel."""

    def __init__(self, B=1, **over):
        super(Acc, self).__init__("f32", B=B, deterministic=True, **over)
        lz = load_golden("loss.npz")
        self.frames = tiny_input().cuda()
        self.all_boxes, self.all_nb = torch.from_numpy(lz["bboxes"]), torch.from_numpy(lz["nbox"])
        self.img1 = self.img[:1]

    def micro(self, frame, s=0, bad=None):
        x = self.frames[frame:frame + 1]
        if bad is not None:
            x = x.clone()
            x[0, 3, 17, 9] = float("nan")
        np.random.seed(100 + s)
        self.tr.one_step(x, self.img1, self.all_boxes[frame:frame + 1], self.all_nb[frame:frame + 1])
        torch.cuda.synchronize()

    def grads(self):
        return self.tr.model.flat_grads.clone()


_PLAIN = {}


def plain(frame, **over):
    """(initial state, gradient, state after) of ONE one_step of a fresh plain trainer on `frame`, seed 100 + frame; computed once."""
    key = (frame, tuple(sorted(over.items())))
    if key not in _PLAIN:
        t = Acc(**over)
        init = t.state()
        t.micro(frame, frame)
        _PLAIN[key] = (init, t.grads(), t.state())
    return _PLAIN[key]


def bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the kernel
SPECIAL = [float("nan"), float("inf"), float("-inf"), -0.0, 1e-40, -3e-42, 0.0]


def _pattern(n, seed, phase):
    """n fp32 values: normals with NaN, +-inf, -0.0, zeros and denormals every third element, in a cycle that starts at `phase` (two
    phases meet as NaN + x, x + NaN, inf + -inf, inf + inf, -0.0 + 0.0, denormal + denormal somewhere in every range of a few dozen)."""
    v = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    for i in range(0, n, 3):
        v[i] = SPECIAL[(i // 3 + phase * (1 + i // 21)) % len(SPECIAL)]
    return v


def test_kernel_every_size_alignment_and_mode():
    ops = pkg("ops")
    lib, stream = pkg("_hip").lib(), pkg("_hip").stream_ptr
    sizes = [0, 1, 3, 4, 5, 1023, 1024, 1025, 2055]
    pad = 8
    canary = 12345.0
    dpat, spat = _pattern(max(sizes), 1, 0).cuda(), _pattern(max(sizes), 2, 1).cuda()
    assert bool(torch.isnan(dpat + spat).any()) and bool(torch.isinf(dpat + spat).any())
    assert bool(((dpat != 0) & (dpat.abs() < 1e-38)).any()), "no denormal survived on the device"
    for n in sizes:
        for doff in range(4):
            for soff in range(4):
                for mode in (0, 1):
                    dbuf = torch.full((n + 2 * pad,), canary, device="cuda")
                    sbuf = torch.full((n + 2 * pad,), -canary, device="cuda")
                    dst, src = dbuf[4 + doff:4 + doff + n], sbuf[4 + soff:4 + soff + n]
                    assert n == 0 or (dst.data_ptr() % 16 == 4 * doff and src.data_ptr() % 16 == 4 * soff)
                    dst.copy_(dpat[:n])
                    src.copy_(spat[:n])
                    want_d, want_s = dbuf.clone(), sbuf.clone()
                    want_d[4 + doff:4 + doff + n] = spat[:n] if mode == 0 else dpat[:n] + spat[:n]      # torch's add, on the device
                    if n:
                        ops.grad_accumulate(dst, src, mode)
                    else:                              # an empty torch tensor has no address: the library itself, at the range's addresses
                        rc = lib.dcf_grad_accumulate(dbuf.data_ptr() + 4 * (4 + doff), sbuf.data_ptr() + 4 * (4 + soff), 0, mode, stream())
                        assert rc == 0
                        ops.grad_accumulate(dst, src, mode)
                    assert torch.equal(bits(dbuf), bits(want_d)), (n, doff, soff, mode)
                    assert torch.equal(bits(sbuf), bits(want_s)), (n, doff, soff, mode)


def test_kernel_rejects_overlap_and_unknown_modes():
    ops, H = pkg("ops"), pkg("_hip")
    buf = torch.arange(200, dtype=torch.float32, device="cuda")
    before = buf.clone()
    other = torch.ones(100, device="cuda")
    for dst, src, mode in ((buf[0:100], buf[50:150], 1), (buf[50:150], buf[0:100], 0), (buf[0:100], buf[99:199], 1), (buf[0:100], buf[0:100], 0),
                           (buf[0:100], other, 2), (buf[0:100], other, -1)):
        with pytest.raises(H.DcfError, match="dcf_grad_accumulate"):
            ops.grad_accumulate(dst, src, mode)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    ops.grad_accumulate(buf[0:100], buf[100:200], 1)                       # touching ranges do not overlap
    assert torch.equal(buf[0:100], before[0:100] + before[100:200]) and torch.equal(buf[100:], before[100:])
    L = H.lib()
    assert L.dcf_grad_accumulate(None, other.data_ptr(), 4, 0, None) == -1 and L.dcf_grad_accumulate(other.data_ptr(), None, 4, 0, None) == -1
    assert L.dcf_grad_accumulate(buf.data_ptr(), other.data_ptr(), -1, 0, None) == -1


# ------------------------------------------------------------------------------------------------ 2. off means off
def test_off_means_off(monkeypatch):
    absent, spelled = Acc(), Acc(grad_accum_steps=1, grad_accum_reduce="mean")
    assert "grad_accum_steps" not in absent.cfg and "grad_accum_reduce" not in absent.cfg
    runs = []
    for t in (absent, spelled):
        t.step(0)                                      # first step: lazy set-up
        runs.append(_record_calls(monkeypatch, t, 1))
        assert t.tr.accum is None and t.tr.accum_buf is None and t.tr.accum_index() == 0
        before = t.state()
        t.tr.finish_window()
        assert _equal3(t.state(), before) and t.tr.optimizer.opt_calls == 2
    assert runs[0] == runs[1]
    assert "dcf_grad_accumulate" not in runs[0] and runs[0].count("dcf_adam_step") == 1
    assert _equal3(absent.state(), spelled.state())
    on = Acc(grad_accum_steps=2)
    assert on.tr.accum_buf is not None and on.tr.accum_buf.numel() == on.tr.model.flat_grads.numel()
    ptr = on.tr.accum_buf.data_ptr()
    on.step(0)
    closing = _record_calls(monkeypatch, on, 1)
    opening = _record_calls(monkeypatch, on, 2)
    assert closing.count("dcf_grad_accumulate") == 1 and closing.count("dcf_adam_step") == 1
    assert [n for n in closing if n != "dcf_grad_accumulate"] == runs[0]
    assert opening.count("dcf_grad_accumulate") == 1
    assert [n for n in opening if n != "dcf_grad_accumulate"] == [n for n in runs[0] if n != "dcf_adam_step"]
    assert on.tr.accum_buf.data_ptr() == ptr
    for bad in (True, 0, -2, 2.0, "2", None):
        with pytest.raises(ValueError, match="grad_accum_steps"):
            Acc(grad_accum_steps=bad)
    with pytest.raises(ValueError, match="grad_accum_reduce"):
        Acc(grad_accum_steps=2, grad_accum_reduce="avg")


# ------------------------------------------------------------------------------------------------ 3. the window, exactly
@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_window_of_two_is_the_left_fold_and_one_adam_call(reduce):
    ops = pkg("ops")
    (init, g1, _), (init2, g2, _) = plain(0), plain(1)
    assert _equal3(init, init2) and not torch.equal(g1, g2)
    t = Acc(grad_accum_steps=2, grad_accum_reduce=reduce)
    assert _equal3(t.state(), init)
    t.micro(0, 0)
    assert _equal3(t.state(), init) and t.tr.accum_index() == 1 and t.tr.optimizer.opt_calls == 0 and t.tr.optimizer.step_count == 0
    assert torch.equal(t.grads(), g1) and torch.equal(t.tr.accum_buf, g1)
    t.micro(1, 1)
    assert t.tr.accum_index() == 0 and t.tr.optimizer.opt_calls == 1 and t.tr.optimizer.step_count == 1
    assert torch.equal(bits(t.grads()), bits(g1 + g2))
    p, m, v = (x.clone() for x in init)
    ops.adam_step(p, g1 + g2, m, v, t.cfg["learning_rate"], t.cfg["beta1"], 0.999, 1e-8, 1, 0.5 if reduce == "mean" else 1.0)
    assert _equal3(t.state(), (p, m, v))
    assert not torch.equal(p, init[0])


def test_window_of_three_adds_in_order():
    (init, g1, _), (_, g2, _) = plain(0), plain(1)
    t = Acc(grad_accum_steps=3)
    for j, frame in enumerate((0, 1, 0)):
        assert t.tr.accum_index() == j and _equal3(t.state(), init)
        t.micro(frame, frame)
    assert t.tr.accum_index() == 0 and t.tr.optimizer.opt_calls == 1
    assert torch.equal(bits(t.grads()), bits((g1 + g2) + g1))


# ------------------------------------------------------------------------------------------------ 4. finish_window
@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_finish_window_after_one_micro_step_is_a_plain_step(reduce):
    init, g1, after = plain(0)
    t = Acc(grad_accum_steps=2, grad_accum_reduce=reduce)
    t.micro(0, 0)
    assert _equal3(t.state(), init) and t.tr.accum_index() == 1
    t.tr.finish_window()
    torch.cuda.synchronize()
    assert t.tr.accum_index() == 0 and t.tr.optimizer.opt_calls == 1
    assert _equal3(t.state(), after) and torch.equal(t.grads(), g1)
    t.tr.finish_window()                               # at a boundary: nothing
    torch.cuda.synchronize()
    assert _equal3(t.state(), after) and t.tr.optimizer.opt_calls == 1 and t.tr.accum_index() == 0


# ------------------------------------------------------------------------------------------------ 5. against the large batch
def test_window_of_two_against_one_batch_of_two():
    """focal draws nothing and weighs every sample alone, so under loss_reduction: mean the batch-2 loss is the mean of the two batch-1
    losses (checked on CPU tensors first) and the batch-2 gradient is (g_1 + g_2) / 2 up to re-association: the bounds of
    tests/test_gpu_dp.py for "N ranks x B frames = one rank x N*B frames"."""
    over = dict(loss_sampling="focal", loss_reduction="mean")
    cfg = tiny_cfg("f32", **over)
    L = pkg("loss").LossTotal(cfg)
    lz = load_golden("loss.npz")
    boxes, nb = torch.from_numpy(lz["bboxes"])[:2], torch.from_numpy(lz["nbox"])[:2]
    Hh, Ww = (int(s) for s in L.anchor_set.shape[2:])
    g = torch.Generator().manual_seed(5)
    cls = torch.softmax(torch.randn(2, 2, 2, Hh * Ww, generator=g), dim=2).reshape(2, 4, Hh, Ww).contiguous()
    reg = torch.rand(2, 14, Hh, Ww, generator=g) - 0.5
    both = float(L(boxes, nb, cls, reg))
    each = [float(L(boxes[b:b + 1], nb[b:b + 1], cls[b:b + 1], reg[b:b + 1])) for b in range(2)]
    print("CPU: batch-2 loss %r, batch-1 losses %r" % (both, each))
    assert each[0] != each[1] and abs(both - 0.5 * (each[0] + each[1])) <= 2e-6 * max(1.0, abs(both))
    big = Acc(B=2, **over)
    big.step(0)
    small = Acc(grad_accum_steps=2, **over)
    small.micro(0, 0)
    small.micro(1, 1)
    a, b = big.grads(), small.grads() * 0.5            # mean over the window, as the optimiser's gscale applies it
    err, top = float((a - b).abs().max()), float(a.abs().max())
    print("gradient: max |batch-2 - window mean| = %g, max |g| = %g, ratio %g" % (err, top, err / top))
    assert top > 0 and err < 1e-5 * top
    pa, pb = big.state()[0], small.state()[0]
    d = (pa - pb).abs()
    lr = big.cfg["learning_rate"]
    frac = float((d > 1e-5 * float(pa.abs().max())).float().mean())
    print("parameters: %.3g apart at most (lr %g), %.2e of them over 1e-5 of the largest" % (float(d.max()), lr, frac))
    assert frac < 1e-3 and float(d.max()) <= 2.5 * lr
    assert float((pa - plain(0)[0][0]).abs().max()) > 0.1 * lr         # the step moved the parameters at all


# ------------------------------------------------------------------------------------------------ 6. guarded step
@pytest.mark.parametrize("bad_at", [1, 2])
def test_nonfinite_micro_step_skips_the_whole_window_once(bad_at):
    t = Acc(loss_scale="dynamic", grad_accum_steps=2)
    t.micro(0, 0)
    t.micro(1, 1)
    after0, a0 = t.state(), t.amp()
    assert a0["found"] == 0 and a0["applied"] == 1 and a0["skipped"] == 0 and a0["scale"] == 65536.0
    s0 = float(t.tr.loss_scale().item())
    t.micro(0, 2, "nan" if bad_at == 1 else None)
    assert float(t.tr.loss_scale().item()) == s0 == 65536.0 and t.amp() == a0       # no amp_update inside the window
    assert _equal3(t.state(), after0)
    t.micro(1, 3, "nan" if bad_at == 2 else None)
    assert not bool(torch.isfinite(t.tr.model.flat_grads).all()), "the bad frame did not reach the window's sum"
    assert _equal3(t.state(), after0)
    a1 = t.amp()
    assert a1["found"] == 1 and a1["scale"] == 32768.0 and a1["skipped"] == 1 and a1["applied"] == 1
    assert t.tr.optimizer.opt_calls == 2 and t.tr.optimizer.step_count == 1
    t.micro(0, 4)
    t.micro(1, 5)
    a2 = t.amp()
    assert a2["applied"] == 2 and a2["skipped"] == 1 and a2["found"] == 0
    ref = Acc(grad_accum_steps=2)                       # never saw the bad window (power-of-two scaling is exact in f32)
    for frame, s in ((0, 0), (1, 1), (0, 4), (1, 5)):
        ref.micro(frame, s)
    assert torch.equal(t.state()[0], ref.state()[0]) and bool(torch.isfinite(t.state()[0]).all())


# ------------------------------------------------------------------------------------------------ 7. recipe
def test_schedule_and_average_tick_per_window():
    O = pkg("optim")
    t = Acc(grad_accum_steps=2, lr_schedule=SCHED, ema_decay=0.9, ema_warmup=True)
    base = t.cfg["learning_rate"]
    rates = [O.lr_at(O.parse_schedule(SCHED), base, k) for k in range(3)]
    assert rates == [0.0, base, base * 0.5]
    snaps = [t.state()[0]]
    seen = [t.tr.learning_rate()]
    for w in range(2):
        t.micro(0, 2 * w)
        seen.append(t.tr.learning_rate())
        assert torch.equal(t.tr.ema_params(), _fold(O, t.cfg, snaps)) and t.tr.optimizer.opt_calls == w
        t.micro(1, 2 * w + 1)
        seen.append(t.tr.learning_rate())
        snaps.append(t.state()[0])
    assert seen == [rates[0], rates[0], rates[1], rates[1], rates[2]]
    assert t.tr.optimizer.opt_calls == 2
    want = _fold(O, t.cfg, snaps)
    assert torch.equal(t.tr.ema_params(), want)
    assert not torch.equal(snaps[2], snaps[1]) and not torch.equal(want, snaps[2])


# ------------------------------------------------------------------------------------------------ 8. checkpoint
def test_checkpoint_inside_a_window_resumes_bitwise(tmp_path):
    a = Acc(grad_accum_steps=2)
    a.micro(0, 0)
    a.tr.save_checkpoint(str(tmp_path / "mid.pt"), epoch=4)
    a.micro(1, 1)
    ck = torch.load(str(tmp_path / "mid.pt"), map_location="cpu")
    assert ck["accum_index"] == 1 and torch.equal(ck["accum"], plain(0)[1].cpu())
    b = Acc(grad_accum_steps=2)
    assert b.tr.load_checkpoint(str(tmp_path / "mid.pt")) == 4
    assert b.tr.accum_index() == 1
    b.micro(1, 1)
    assert _equal3(a.state(), b.state()) and torch.equal(bits(a.grads()), bits(b.grads())) and b.tr.accum_index() == 0
    a.tr.save_checkpoint(str(tmp_path / "edge.pt"))    # at a boundary: the index, no accumulator
    ck = torch.load(str(tmp_path / "edge.pt"), map_location="cpu")
    assert ck["accum_index"] == 0 and "accum" not in ck
    c = Acc()                                           # written with accumulation off: no keys, loads at a boundary
    c.micro(0, 0)
    c.tr.save_checkpoint(str(tmp_path / "plain.pt"))
    ck = torch.load(str(tmp_path / "plain.pt"), map_location="cpu")
    assert "accum_index" not in ck and "accum" not in ck
    d = Acc(grad_accum_steps=2)
    d.tr.load_checkpoint(str(tmp_path / "plain.pt"))
    assert d.tr.accum_index() == 0 and _equal3(d.state(), c.state()) and d.tr.optimizer.opt_calls == 1
    with pytest.raises(ValueError, match="accumulation window"):
        c.tr.load_checkpoint(str(tmp_path / "mid.pt"))


# ------------------------------------------------------------------------------------------------ 9. captured graphs
def test_hip_graphs_batch1_two_windows_equal_eager():
    runs = {}
    for graphs in (True, False):
        t = Acc(hip_graphs=graphs, grad_accum_steps=2)
        assert t.tr.model.graphs_wanted(1) == graphs
        out = []
        for w in range(2):
            t.micro(0, 2 * w)
            t.micro(1, 2 * w + 1)
            out.append((t.grads(),) + t.state())
        runs[graphs] = out
    for w in range(2):
        for name, a, b in zip(("g", "p", "m", "v"), runs[True][w], runs[False][w]):
            print("window %d %s: max |graphs - eager| = %g" % (w, name, float((a - b).abs().max())))
    for w in range(2):
        for a, b in zip(runs[True][w], runs[False][w]):
            assert torch.equal(a, b), w
    assert not torch.equal(runs[False][1][1], runs[False][0][1])


# ------------------------------------------------------------------------------------------------ 10. one collective per window
@pytest.mark.parametrize("bucket", ["f32", "bf16"])
def test_one_collective_per_window(tmp_path, monkeypatch, bucket):
    import torch.distributed as dist
    alone = Acc(grad_accum_steps=2)
    alone.micro(0, 0)
    alone.micro(1, 1)
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "pg"), rank=0, world_size=1)
    try:
        t = Acc(grad_accum_steps=2, overlap_allreduce="force", grad_bucket_dtype=bucket)
        reduced, ranges = [], []
        real_reduce, real_ready = dist.all_reduce, t.tr._bucket_ready

        def counting(tensor, *a, **k):
            reduced.append(tensor.numel())
            return real_reduce(tensor, *a, **k)

        def ready(rs):
            ranges.extend((a, b) for a, b in rs if b > a)
            return real_ready(rs)

        monkeypatch.setattr(dist, "all_reduce", counting)
        t.tr._bucket_ready = ready
        t.micro(0, 0)
        assert reduced == [] and ranges == [] and t.tr.accum_index() == 1
        t.micro(1, 1)
        n = t.tr.model.flat_grads.numel()
        ranges.sort()
        assert ranges and ranges[0][0] == 0 and ranges[-1][1] == n and all(x[1] == y[0] for x, y in zip(ranges, ranges[1:]))
        assert len(reduced) == len(ranges) and sum(reduced) == n and t.tr._reduced == n
        assert bool(t.tr._widen) == (bucket == "bf16")
        if bucket == "f32":
            assert torch.equal(bits(t.grads()), bits(alone.grads())) and _equal3(t.state(), alone.state())
        else:
            assert torch.equal(bits(t.grads()), bits(alone.grads().to(torch.bfloat16).float()))
            assert not torch.equal(t.grads(), alone.grads())
    finally:
        dist.destroy_process_group()
