"""EMA of the parameters, host side (no GPU): the new C entries are declared, listed and exported, the decay
schedule ``ema_decay_at`` is the stated formula, and ``TrainStep``'s argument errors come before it touches a device."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tdx_adam_ema_step", "tdx_adam_ema_step_dev", "tdx_adam_ema_step_clip", "tdx_swap_f32")


def test_new_symbols_declared_listed_and_exported():
    import tiny_diffusion_amd._lib as L

    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS, name
        assert getattr(L.lib, name).argtypes is not None, name   # bound: the library exports it
    assert L.lib.tdx_version() == 400   # the ABI only grows


def test_decay_without_warmup_is_the_decay():
    from tiny_diffusion_amd.train import ema_decay_at

    for k in (0, 1, 1000):
        assert ema_decay_at(k, 0.9999, False) == 0.9999
        assert ema_decay_at(k, 0.5, False) == 0.5


def test_decay_warmup_formula():
    from tiny_diffusion_amd.train import ema_decay_at

    d = 0.9999
    assert ema_decay_at(0, d, True) == 0.1
    assert ema_decay_at(1, d, True) == 2 / 11
    first = next(k for k in range(200000) if (1 + k) / (10 + k) >= d)
    assert ema_decay_at(first - 1, d, True) < d
    for k in (first, first + 1, 10 * first):
        assert ema_decay_at(k, d, True) == d
    prev = 0.0
    for k in range(100001):
        cur = ema_decay_at(k, d, True)
        assert prev <= cur <= d, k
        prev = cur
    assert prev == d


class _OnDevice:
    """Enough of a CUDA-resident model for TrainStep's argument checks, which come before it touches parameters."""

    def __init__(self, model):
        self._arch, self.num_classes = model._arch, model.num_classes


@pytest.mark.parametrize("decay", [-0.1, 1.5, float("nan"), "0.9", True])
def test_ema_decay_outside_unit_interval(decay):
    from tiny_diffusion_amd.conditional_diffusion import ForwardProcess, NoiseModel
    from tiny_diffusion_amd.train import TrainStep

    with pytest.raises(ValueError, match="ema_decay"):
        TrainStep(_OnDevice(NoiseModel()), ForwardProcess(), ema_decay=decay)


def test_ema_warmup_needs_a_decay():
    from tiny_diffusion_amd.conditional_diffusion import ForwardProcess, NoiseModel
    from tiny_diffusion_amd.train import TrainStep

    with pytest.raises(ValueError, match="ema_decay"):
        TrainStep(_OnDevice(NoiseModel()), ForwardProcess(), ema_warmup=True)
