"""The property the shared training-step base (tiny_diffusion_amd/_flat_step.py) relies on: an optimizer entry that
derives its step scalars from ``lr``, the betas and the step number, and the graph-capturable entry that reads them
from a device tensor filled by ``adam_hyper``, update bit-identically.  n = 1000 is no multiple of the 256-thread block
(a ragged final block); steps 1, 2 and 1000 cover the first bias corrections and a late one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, LR, B1, B2, EPS = 1000, 1e-3, 0.9, 0.999, 1e-8
STEPS = (1, 2, 1000)


def _state(k, with_ema=False):
    """Random p, g, m, v (v >= 0) [, e] on the GPU, twice: one copy per entry under comparison."""
    g = torch.Generator().manual_seed(100 + k)
    t = [torch.randn(N, generator=g), torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g),
         0.01 * torch.rand(N, generator=g)]
    if with_ema:
        t.append(torch.randn(N, generator=g))
    return [x.cuda() for x in t], [x.cuda() for x in t]


def _ptrs(ts):
    return [x.data_ptr() for x in ts]


def _same(a, b, which):
    torch.cuda.synchronize()
    return all(torch.equal(a[i], b[i]) for i in which)


def _hyper(k, gscale=1.0, ema_a=None):
    from tiny_diffusion_amd._flat_step import adam_hyper

    h = torch.tensor(adam_hyper(LR, (B1, B2), k, gscale, ema_a), dtype=torch.float32).cuda()
    torch.cuda.synchronize()
    return h


@pytest.mark.parametrize("k", STEPS)
def test_adam_step_and_its_device_scalar_form_agree_bit_for_bit(k):
    from tiny_diffusion_amd._lib import check, lib

    st = torch.cuda.current_stream().cuda_stream
    a, b = _state(k)
    h = _hyper(k)
    check(lib.tdx_adam_step(*_ptrs(a), N, LR, B1, B2, EPS, k, 1.0, st), "tdx_adam_step")
    check(lib.tdx_adam_step_dev(*_ptrs(b), N, h.data_ptr(), B1, B2, EPS, st), "tdx_adam_step_dev")
    assert _same(a, b, (0, 2, 3))
    assert not torch.equal(a[0], _state(k)[0][0])      # (the step did move the parameters)


@pytest.mark.parametrize("k", STEPS)
def test_adam_ema_step_and_its_device_scalar_form_agree_bit_for_bit(k):
    from tiny_diffusion_amd._lib import check, lib
    from tiny_diffusion_amd.train import ema_decay_at

    st = torch.cuda.current_stream().cuda_stream
    ema_a = 1.0 - ema_decay_at(k - 1, 0.999, True)
    a, b = _state(k, with_ema=True)
    order = lambda s: _ptrs(s[:4]) + [s[4].data_ptr()]     # noqa: E731
    h = _hyper(k, ema_a=ema_a)
    check(lib.tdx_adam_ema_step(*order(a), N, LR, B1, B2, EPS, k, 1.0, ema_a, st), "tdx_adam_ema_step")
    check(lib.tdx_adam_ema_step_dev(*order(b), N, h.data_ptr(), B1, B2, EPS, st), "tdx_adam_ema_step_dev")
    assert _same(a, b, (0, 2, 3, 4))
    assert not torch.equal(a[4], _state(k, with_ema=True)[0][4])      # (the average did move)


@pytest.mark.parametrize("k", STEPS)
def test_adam_step_clip_host_and_device_scalars_agree_bit_for_bit(k):
    from tiny_diffusion_amd._lib import check, lib

    st = torch.cuda.current_stream().cuda_stream
    a, b = _state(k)
    assert float(a[1].norm()) > 20.0                   # |g| ~ sqrt(1000): max_norm = 0.5 clips
    scratch = torch.empty(lib.tdx_adam_clip_scratch_bytes(), dtype=torch.uint8, device="cuda")
    h = _hyper(k)
    check(lib.tdx_adam_step_clip(*_ptrs(a), N, LR, B1, B2, EPS, k, 1.0, 0.5, None, scratch.data_ptr(), st),
          "tdx_adam_step_clip")
    check(lib.tdx_adam_step_clip(*_ptrs(b), N, LR, B1, B2, EPS, k, 1.0, 0.5, h.data_ptr(), scratch.data_ptr(), st),
          "tdx_adam_step_clip")
    assert _same(a, b, (0, 2, 3))
    # clipping took effect: the second moment grew by (1 - b2) (c g)^2 with c = 0.5 / |g| << 1, not by (1 - b2) g^2
    v0 = _state(k)[0][3]
    assert float((a[3] - B2 * v0).max()) < 1e-3 * float(((1 - B2) * a[1] ** 2).max())
