"""Host checks of the step guard that need no GPU: the Adam constructor's rule for skip_nonfinite, skip_stats()
before build, fit's max_consecutive_skips refused before anything is launched, and the optimizer's half of a
checkpoint with and without the guard's counters (on CPU tensors: build and the checkpoint helpers launch nothing)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from vqa_module import keras_fit_feed
from vqa_optim import SKIP_STATS, Adam
from vqa_train import adam_from_checkpoint, adam_state, check_skip_limit, raise_on_skips, set_adam_state


def _store(n=12):
    return SimpleNamespace(flat=torch.arange(n, dtype=torch.float32), size=n, offsets={"a": (0, (8,)), "b": (8, (4,))},
                           from_layout=lambda t, layout, what: t)


def _built(**kw):
    opt = Adam(**kw)
    opt.build(_store())
    return opt


# ---- the constructor
def test_the_guard_is_off_by_default_and_kept_when_set():
    assert Adam().skip_nonfinite is False
    assert Adam(skip_nonfinite=True).skip_nonfinite is True
    assert Adam(skip_nonfinite=np.True_).skip_nonfinite is True
    assert Adam(skip_nonfinite=False).skip_nonfinite is False


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0, [True]])
def test_skip_nonfinite_must_be_a_bool(bad):
    with pytest.raises(ValueError, match="skip_nonfinite"):
        Adam(skip_nonfinite=bad)


# ---- skip_stats
def test_skip_stats_needs_the_guard_and_a_built_optimizer():
    with pytest.raises(RuntimeError, match="skip_stats"):
        Adam(skip_nonfinite=True).skip_stats()          # not built
    with pytest.raises(RuntimeError, match="skip_stats"):
        _built().skip_stats()                            # built, guard off
    assert _built().skipped is None and _built().step_ok is None


def test_skip_stats_are_views_of_buffers_allocated_once_in_build():
    opt = _built(skip_nonfinite=True)
    st = opt.skip_stats()
    assert tuple(st) == SKIP_STATS == ("skipped_steps", "consecutive_skipped", "last_step_ok")
    assert all(v.dim() == 0 for v in st.values())
    assert [int(v) for v in st.values()] == [0, 0, 1]
    assert opt.skipped.dtype == torch.int64 and opt.step_ok.dtype == torch.int32
    opt.skipped.copy_(torch.tensor([5, 2]))
    opt.step_ok.fill_(0)
    assert [int(v) for v in st.values()] == [5, 2, 0]    # the views follow the buffers: nothing was copied
    assert opt.skip_stats()["skipped_steps"].data_ptr() == opt.skipped.data_ptr()


# ---- max_consecutive_skips
def test_a_skip_limit_needs_a_guarded_optimizer_before_any_launch():
    launched = []
    model = SimpleNamespace(optimizer=Adam(), reset_metrics=lambda: launched.append("reset"),
                            train_step=lambda feed: launched.append("step"))
    feed = SimpleNamespace(steps_per_epoch=3)
    with pytest.raises(ValueError, match="max_consecutive_skips"):
        keras_fit_feed(model, feed, epochs=1, max_consecutive_skips=2)
    with pytest.raises(ValueError, match="max_consecutive_skips"):
        keras_fit_feed(SimpleNamespace(optimizer=None), feed, epochs=1, max_consecutive_skips=2)
    assert launched == []
    check_skip_limit(Adam(), None)                        # no limit: any optimizer
    check_skip_limit(None, None)
    check_skip_limit(Adam(skip_nonfinite=True), 1)


@pytest.mark.parametrize("bad", [0, -1, 1.5, True, "2"])
def test_a_skip_limit_is_an_integer_of_at_least_one(bad):
    with pytest.raises(ValueError, match="max_consecutive_skips"):
        check_skip_limit(Adam(skip_nonfinite=True), bad)


def test_the_epoch_end_check_names_the_epoch_and_both_counts():
    opt = _built(skip_nonfinite=True)
    opt.skipped.copy_(torch.tensor([7, 2]))
    raise_on_skips(opt, None, 0)
    raise_on_skips(opt, 3, 0)                             # 2 in a row < 3
    with pytest.raises(FloatingPointError) as e:
        raise_on_skips(opt, 2, 4)
    msg = str(e.value)
    assert "epoch 5" in msg and "2 train steps in a row" in msg and "7 steps skipped in all" in msg


def test_fit_reads_the_counters_at_epoch_ends_only():
    """keras_fit_feed with a limit: the fake train_step skips every step; the error comes after the whole epoch."""
    opt = _built(skip_nonfinite=True)
    steps = []

    def train_step(feed):
        steps.append(1)
        opt.skipped += 1

    model = SimpleNamespace(optimizer=opt, reset_metrics=lambda: None, train_step=train_step,
                            results=lambda: {"loss": torch.tensor(0.0)})
    with pytest.raises(FloatingPointError, match="epoch 1"):
        keras_fit_feed(model, SimpleNamespace(steps_per_epoch=5), epochs=3, max_consecutive_skips=2)
    assert len(steps) == 5


# ---- checkpoints
def test_the_counters_travel_in_the_optimizers_state():
    a = _built(skip_nonfinite=True)
    a.skipped.copy_(torch.tensor([4, 1]))
    a.step_ok.fill_(0)
    a.iterations.fill_(9)
    sd = adam_state(a)
    assert sd["adam_skipped"] == [4, 1] and all(type(c) is int for c in sd["adam_skipped"])
    sd = adam_from_checkpoint(sd, _store(), None, "file")
    assert sd["adam_skipped"] == [4, 1]
    b = _built(skip_nonfinite=True)
    set_adam_state(b, sd, torch.device("cpu"))
    assert [int(v) for v in b.skip_stats().values()] == [int(v) for v in a.skip_stats().values()] == [4, 1, 0]
    assert int(b.iterations) == 9


def test_a_state_without_counters_loads_as_zeros():
    plain = _built()
    sd = adam_state(plain)
    assert "adam_skipped" not in sd
    assert "adam_skipped" not in adam_from_checkpoint(sd, _store(), None, "file")
    b = _built(skip_nonfinite=True)
    b.skipped.copy_(torch.tensor([3, 3]))
    b.step_ok.fill_(0)
    set_adam_state(b, sd, torch.device("cpu"))
    assert [int(v) for v in b.skip_stats().values()] == [0, 0, 1]


def test_an_optimizer_without_the_guard_ignores_the_counters():
    a = _built(skip_nonfinite=True)
    a.skipped.copy_(torch.tensor([2, 0]))
    a.m.fill_(0.5)
    plain = _built()
    set_adam_state(plain, adam_state(a), torch.device("cpu"))
    assert plain.skipped is None and plain.step_ok is None and torch.equal(plain.m, a.m)
