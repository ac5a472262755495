"""CPU suite: gradient accumulation's host side (train.parse_accum_config / train.window_factor) -- the accepted
and the rejected forms of grad_accum_steps / grad_accum_reduce, the defaults, and the factor a window multiplies into the optimiser's
gradient scale, a short window closed by finish_window included."""
import pytest

from _util import pkg


def test_absent_and_one_are_off():
    T = pkg("train")
    assert T.parse_accum_config({}) is None
    assert T.parse_accum_config({"grad_accum_steps": 1}) is None
    assert T.parse_accum_config({"grad_accum_steps": 1, "grad_accum_reduce": "sum"}) is None
    assert T.parse_accum_config({"grad_accum_reduce": "mean"}) is None


def test_accepted_forms_and_the_default_reduction():
    T = pkg("train")
    assert T.parse_accum_config({"grad_accum_steps": 2}) == {"steps": 2, "reduce": "mean"}
    assert T.parse_accum_config({"grad_accum_steps": 4, "grad_accum_reduce": "mean"}) == {"steps": 4, "reduce": "mean"}
    assert T.parse_accum_config({"grad_accum_steps": 64, "grad_accum_reduce": "sum"}) == {"steps": 64, "reduce": "sum"}
    assert T.parse_accum_config({"grad_accum_steps": 3, "grad_accum_reduce": " Sum "}) == {"steps": 3, "reduce": "sum"}
    got = T.parse_accum_config({"grad_accum_steps": 2})
    assert type(got["steps"]) is int


@pytest.mark.parametrize("k", [True, False, 0, -1, -4, 2.0, 1.5, "2", None, [2], float("nan")])
def test_rejected_steps(k):
    T = pkg("train")
    with pytest.raises(ValueError, match="grad_accum_steps"):
        T.parse_accum_config({"grad_accum_steps": k})


@pytest.mark.parametrize("red", ["avg", "", None, 1, True, ["mean"], "mean,sum"])
@pytest.mark.parametrize("k", [None, 1, 2])
def test_rejected_reductions_whether_on_or_off(red, k):
    T = pkg("train")
    cfg = {"grad_accum_reduce": red}
    if k is not None:
        cfg["grad_accum_steps"] = k
    with pytest.raises(ValueError, match="grad_accum_reduce"):
        T.parse_accum_config(cfg)


def test_window_factor():
    """mean: 1 / j for the j micro-steps the window really holds -- k for a full one, fewer when finish_window closes it early; sum: 1.
    The trainer passes (1 / (world * premul)) * factor as the optimiser's gradient scale."""
    T = pkg("train")
    mean, plain = T.parse_accum_config({"grad_accum_steps": 4}), T.parse_accum_config({"grad_accum_steps": 4, "grad_accum_reduce": "sum"})
    assert [T.window_factor(mean, j) for j in (1, 2, 3, 4)] == [1.0, 0.5, 1.0 / 3, 0.25]
    assert [T.window_factor(plain, j) for j in (1, 2, 3, 4)] == [1.0, 1.0, 1.0, 1.0]
    assert T.window_factor(None, 1) == 1.0                                  # accumulation off
    assert (1.0 / (1 * 1.0)) * T.window_factor(mean, 2) == 0.5              # one rank, no premultiplier, a full window of two
    assert (1.0 / (1 * 1.0)) * T.window_factor(mean, 1) == 1.0              # ... and a window of one closed by finish_window
    for j in (0, -1, True, 1.0):
        with pytest.raises(ValueError):
            T.window_factor(mean, j)
