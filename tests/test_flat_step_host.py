"""The shared base of the fused training steps (tiny_diffusion_amd/_flat_step.py), host side (no GPU): ``adam_hyper``
is the C entry's arithmetic bit for bit, the capture protocol's three states, the workspace cache's eviction rule and
``_check_objective`` on every class that has an objective."""
import math

import numpy as np
import pytest
import torch

from tiny_diffusion_amd._flat_step import FlatStep, adam_hyper


def _c_scalars(lr, b1, b2, k):
    """What tdx_adam_step computes from its ``float`` arguments: ``(float)(lr / (1 - pow((double)beta1, step)))`` and
    ``(float)(1 / sqrt(1 - pow((double)beta2, step)))``."""
    return (np.float32(np.float32(lr) / (1 - np.float32(b1).astype(float) ** k)),
            np.float32(1 / math.sqrt(1 - float(np.float32(b2)) ** k)))


@pytest.mark.parametrize("lr,b1,b2", [(1e-3, .9, .999), (3e-4, .9, .99), (1e-4, .5, .9)])
def test_adam_hyper_is_the_c_arithmetic_bit_for_bit(lr, b1, b2):
    for k in range(1, 2001):
        h = adam_hyper(lr, (b1, b2), k, 0.25)
        want = _c_scalars(lr, b1, b2, k)
        assert len(h) == 3 and h[2] == 0.25
        assert np.float32(h[0]) == want[0] and np.float32(h[1]) == want[1], k
    assert adam_hyper(lr, (b1, b2), 7, 1.0, ema_a=0.123456789)[3] == 0.123456789
    assert adam_hyper(lr, (b1, b2), 7, 1.0, ema_a=0.5)[:3] == adam_hyper(lr, (b1, b2), 7, 1.0)


def test_double_precision_formula_is_told_apart():
    """Negative control: the formula on Python doubles (betas not rounded to fp32 first) differs from the C expression
    at the very first step, so the test above can tell the two apart."""
    lr, b1, b2, k = 1e-3, .9, .999, 1
    old = (np.float32(lr / (1.0 - b1 ** k)), np.float32(1.0 / math.sqrt(1.0 - b2 ** k)))
    assert old != _c_scalars(lr, b1, b2, k)


class _FakeGraph:
    def __init__(self, log):
        self.log = log

    def replay(self):
        self.log.append("replay")


class _Step(FlatStep):
    """A subclass whose capture and replay only record calls (no CUDA graph is opened)."""

    def __init__(self, **kw):
        self._init_optimizer(1e-3, (0.9, 0.999), 1e-8, None, **kw)
        self.device = torch.device("cpu")
        self.diffusion = None
        self.loss = "loss"
        self.log = []

    def _eager(self, hyper=None):
        self.log.append("eager" if hyper is None else "captured body")
        self.step_count += 1
        return self.loss

    def _alloc_static(self, B):
        self.log.append(f"alloc {B}")
        self._gws = self._workspace(B)

    def _static_step(self, hyper):
        assert hyper is self._hyper
        self._eager(hyper)

    def _capture(self, body):
        body()
        return _FakeGraph(self.log)

    def _workspace_floats(self, B):
        return 8 * B

    def step(self, B):
        if not self._graph_ready((B,), B):
            return self._eager()
        return self._replay()


def test_graph_protocol_eager_capture_replay():
    s = _Step()
    n = 0

    def call(B, want):
        nonlocal n
        s.log.clear()
        assert s.step(B) == "loss"
        n += 1
        assert s.log == want and s.step_count == n, (s.log, s.step_count, n)

    call(4, ["eager"])
    assert s._graph is None
    call(4, ["alloc 4", "captured body", "replay"])
    g = s._graph
    assert g is not None and s._hyper.numel() == 3 and s._gws is s._ws[4]
    call(4, ["replay"])
    call(4, ["replay"])
    assert s._graph is g
    want = torch.tensor(adam_hyper(1e-3, (0.9, 0.999), 4, 1.0), dtype=torch.float32)
    assert torch.equal(s._hyper, want)                 # the scalars of the step just replayed
    call(8, ["eager"])                                 # another key: the graph and its hold on the workspace go
    assert s._graph is None and s._gws is None
    call(8, ["alloc 8", "captured body", "replay"])
    assert s._graph is not None and s._gws is s._ws[8]
    call(4, ["eager"])                                 # back: not remembered
    assert s._graph is None
    call(4, ["alloc 4", "captured body", "replay"])
    s._check_objective = lambda *a: None               # (no diffusion here: only the drop is under test)
    s._upload_weights = lambda: None
    s.set_objective()
    assert s._graph is None and s._graph_key is None and s._gws is None
    call(4, ["eager"])
    call(4, ["alloc 4", "captured body", "replay"])


def test_graph_hyper_has_a_fourth_scalar_with_an_average():
    s = _Step(ema_decay=0.999, ema_warmup=True)
    s.ema = torch.zeros(1)
    for _ in range(3):
        s.step(2)
    assert s.step_count == 3 and s._hyper.numel() == 4
    assert float(s._hyper[3]) == np.float32(1.0 - 3 / 12)      # 1 - min(decay, (1 + k) / (10 + k)) at k = 2


def test_workspace_cache_keeps_four_and_never_evicts_the_graphs():
    s = _Step()
    for B in (1, 2, 3, 4, 5):
        assert s._workspace(B).numel() == 8 * B
        assert len(s._ws) <= 4
    assert s._workspace(5) is s._workspace(5)          # cached
    s = _Step()
    s.step(16), s.step(16)
    held = s._gws
    assert held is not None and held.numel() == 128
    for B in range(1, 14):                             # several rounds of eviction
        s._workspace(B)
        assert len(s._ws) <= 4 and s._ws.get(16) is held and s._gws is held
    assert s._workspace(16) is held


def _bare(cls):
    from tiny_diffusion_amd.schedule import ForwardProcess

    step = object.__new__(cls)
    step.diffusion = ForwardProcess(num_timesteps=20)
    return step


def test_check_objective_on_every_class_with_an_objective():
    from tiny_diffusion_amd.diffusion_transformer import TransformerTrainStep
    from tiny_diffusion_amd.train import TrainStep

    for cls in (TrainStep, TransformerTrainStep):
        assert cls._check_objective is FlatStep._check_objective
        step = _bare(cls)
        step._check_objective("v", "min_snr", 3.0)
        for bad in (("x0", None, 5.0), ("eps", "snr", 5.0), ("eps", "min_snr", 0), ("eps", torch.ones(19), 5.0)):
            with pytest.raises(ValueError):
                step._check_objective(*bad)
            assert (step.prediction, step.loss_weighting, step.snr_gamma, step._w_cpu) == ("v", "min_snr", 3.0, None)
        step._check_objective("eps", torch.ones(20), 5.0)
        assert step.loss_weighting == "table" and torch.equal(step._w_cpu, torch.ones(20))
