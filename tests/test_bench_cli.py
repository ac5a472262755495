"""bench.py's command line on the host side: which legs a plain run and a --full run schedule after the timed steps, the output
dump of --dump-outputs (format, size bound, a sample that is the same from run to run), and argument checks that end the run
before it touches the GPU."""
import argparse
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _args(**kw):
    base = dict(full=False, no_other_leg=False, no_batch_sweep=False, no_roofline=False, no_cpu_baseline=False)
    base.update(kw)
    return argparse.Namespace(**base)


def test_plain_run_schedules_no_extra_leg():
    import bench
    for ws in (1, 2):
        assert not any(bench.extra_legs(_args(), ws).values())
    # the --no-* flags never switch anything on
    assert not any(bench.extra_legs(_args(no_other_leg=True, no_roofline=True), 1).values())


def test_full_run_schedules_every_leg_unless_switched_off():
    import bench
    assert bench.extra_legs(_args(full=True), 1) == {"other_leg": True, "batch_sweep": True, "roofline": True, "cpu_baseline": True}
    # several ranks: only the instrumented roofline steps (they contain the all-reduce every rank must join)
    assert bench.extra_legs(_args(full=True), 2) == {"other_leg": False, "batch_sweep": False, "roofline": True, "cpu_baseline": False}
    legs = bench.extra_legs(_args(full=True, no_cpu_baseline=True, no_batch_sweep=True), 1)
    assert legs == {"other_leg": True, "batch_sweep": False, "roofline": True, "cpu_baseline": False}
    assert not bench.extra_legs(_args(full=True, no_other_leg=True, no_roofline=True), 1)["other_leg"]
    assert not bench.extra_legs(_args(full=True, no_other_leg=True, no_roofline=True), 1)["roofline"]


def _fake_trainer(n_params, n_buf, seed):
    g = torch.Generator().manual_seed(seed)
    model = SimpleNamespace(flat_params=torch.randn(n_params, generator=g), flat_grads=torch.randn(n_params, generator=g),
                            _bufflat=torch.randn(n_buf, generator=g))
    opt = SimpleNamespace(m=torch.randn(n_params, generator=g), v=torch.rand(n_params, generator=g))
    return SimpleNamespace(model=model, optimizer=opt, loss_value=torch.tensor(3.25))


def test_dump_outputs_writes_float32_arrays_and_a_fixed_sample(tmp_path):
    import bench
    tr = _fake_trainer(5000, 40, 1)
    names = bench.dump_outputs(tr, str(tmp_path / "a"), sample=1000, seed=0)
    assert names == ["adam_m", "adam_v", "buffers", "grads", "loss", "params"]
    arrs = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in names}
    assert all(a.dtype == np.float32 and a.ndim == 1 for a in arrs.values())
    assert arrs["loss"].tolist() == [3.25]
    assert np.array_equal(arrs["buffers"], tr.model._bufflat.numpy())           # short arenas are written whole
    assert arrs["params"].shape == (1000,) and arrs["grads"].shape == (1000,)
    # the sample: sorted distinct indices, the same for every arena of one length and for every run
    idx = np.sort(np.random.default_rng(0).choice(5000, 1000, replace=False))
    assert np.unique(idx).size == 1000
    assert np.array_equal(arrs["params"], tr.model.flat_params.numpy()[idx])
    assert np.array_equal(arrs["adam_v"], tr.optimizer.v.numpy()[idx])
    bench.dump_outputs(_fake_trainer(5000, 40, 1), str(tmp_path / "b"), sample=1000, seed=0)
    for n in names:
        assert np.array_equal(arrs[n], np.load(str(tmp_path / "b" / (n + ".npy"))))


def test_dump_outputs_stays_within_64_mb():
    import bench
    # at most DUMP_SAMPLE float32 values for each of the five arenas, one for the loss, a 128-byte header per file
    assert 5 * bench.DUMP_SAMPLE * 4 + 4 + 6 * 128 <= 64 * 2 ** 20


def test_seeded_state_puts_the_set_up_state_back_in_place():
    import bench
    tr = _fake_trainer(300, 20, 2)
    tr.optimizer.step_count = 0
    tr.model._backend = SimpleNamespace(amax=torch.zeros(8))
    arenas = lambda: (tr.model.flat_params, tr.optimizer.m, tr.optimizer.v, tr.model._bufflat)
    want = [t.clone() for t in arenas()]
    where = [t.data_ptr() for t in arenas()]
    st = bench.SeededState(tr)
    for t in arenas() + (tr.model._backend.amax,):
        t.add_(1.0)
    tr.optimizer.step_count = 7
    st.restore()
    assert all(torch.equal(a, b) for a, b in zip(arenas(), want)) and [t.data_ptr() for t in arenas()] == where
    assert tr.optimizer.step_count == 0 and not tr.model._backend.amax.any()


def test_bad_step_counts_end_the_run_before_the_gpu():
    for argv in (["--steps", "0"], ["--warmup", "-1"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert p.returncode == 2 and "must be" in p.stderr and not p.stdout.strip(), (argv, p.returncode, p.stderr[-500:])
