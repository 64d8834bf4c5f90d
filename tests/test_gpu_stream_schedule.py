"""The three-stream schedule of the training step (csrc/unet.hip: forks, joins, the stream waits the caller's stream
leaves out because an earlier wait implies them, the slab reduction enqueued behind the skip branch's adjoint) computes
what one stream computes, bit for bit: the kernels and every summation order are the same, only the order of
independent launches differs.  A dependency dropped by the schedule shows as a changed bit - on a chip whose streams
are loaded unevenly rather than on an idle one, hence the junk kernels of the second test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.weights import make_state_dict, make_state_dict_laion  # noqa: E402


def _model(kind, seed=3):
    if kind == "laion":
        from tiny_diffusion_amd.conditional_diffusion_laion import NoiseModel
        m = NoiseModel(time_dim=768)
        m.load_state_dict(make_state_dict_laion(seed), strict=True)
    elif kind == "cond":
        from tiny_diffusion_amd.conditional_diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict(seed, True), strict=True)
    else:
        from tiny_diffusion_amd.diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict(seed, False), strict=True)
    return m.cuda().train()


def _inputs(kind, B, steps, seed=11):
    g = torch.Generator().manual_seed(seed)
    shape = (4, 32, 32) if kind == "laion" else (1, 28, 28)
    x0 = (torch.rand(steps, B, *shape, generator=g) * 2 - 1).cuda()
    t = torch.randint(0, 1000, (steps, B), generator=g).cuda()
    if kind == "laion":
        y = torch.randn(steps, B, 768, generator=g).cuda()
    elif kind == "cond":
        y = torch.randint(0, 10, (steps, B), generator=g).cuda()
    else:
        y = None
    return x0, t, y


def _train(kind, B, steps, stream_mode, before_step=None):
    """`steps` consecutive TrainStep steps from the same start; what the last one left behind."""
    from tiny_diffusion_amd.diffusion import ForwardProcess
    from tiny_diffusion_amd.train import TrainStep

    m = _model(kind)
    if stream_mode is not None:
        m._stream_mode = stream_mode
    ts = TrainStep(m, ForwardProcess(), lr=1e-3, philox_seed=99)
    x0, t, y = _inputs(kind, B, steps)
    for s in range(steps):
        if before_step is not None:
            before_step()
        loss = ts.step(x0[s], None if y is None else y[s], t=t[s])
    torch.cuda.synchronize()
    out = {"loss": loss.clone(), "params": ts.flat_param.clone(), "grads": ts.flat_grad.clone()}
    for k, b in m.named_buffers():
        out["buffer " + k] = b.clone()
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("kind,B", [("uncond", 16), ("cond", 16), ("laion", 16), ("uncond", 48)])
def test_three_stream_schedule_equals_single_stream(kind, B):
    """Three consecutive steps (the pack tail and the slab ping-pong of step n meet step n + 1) with the network's
    default schedule and with `_stream_mode = 0` (everything on the caller's stream): loss, every parameter, every
    gradient of the last step and every BatchNorm buffer are torch.equal.  B = 48 is the smallest batch of
    test_training_step_is_bitwise_reproducible: the Winograd weight gradient and both slab buffers are in play.
    (The equality held before the schedule was re-ordered as well: profiles/r12_event_chain_ab.txt, section 3.)"""
    default = _train(kind, B, 3, None)
    single = _train(kind, B, 3, 0)
    assert torch.isfinite(default["loss"]).all() and default["grads"].abs().max() > 0
    _assert_same(default, single, f"{kind} B={B}")


def test_schedule_is_bitwise_stable_under_uneven_load():
    """The B = 16 MNIST step ten times from the same state, with a bandwidth-heavy junk kernel enqueued in front of it:
    none (repetition 0), on the caller's stream (odd repetitions), on a fresh stream (even ones), so that the caller's
    stream and the helpers meet in another order every time.  All ten results are bit-identical."""
    junk = torch.zeros(1 << 26, device="cuda")
    keep = []

    def load(rep):
        if rep == 0:
            return None
        if rep & 1:
            return lambda: [junk.add_(1.0) for _ in range(2 + rep // 2)]
        s = torch.cuda.Stream()
        keep.append(s)

        def on_side():
            with torch.cuda.stream(s):
                for _ in range(2 + rep // 2):
                    junk.add_(1.0)
        return on_side

    first = None
    for rep in range(10):
        torch.cuda.synchronize()
        got = _train("uncond", 16, 1, None, load(rep))
        if first is None:
            first = got
        else:
            _assert_same(first, got, f"repetition {rep}")


def test_split_backward_with_join_equals_one_call():
    """tdx_unet_backward as stages [0, 5) then [5, 15) with tdx_unet_backward_join on another stream after each part,
    against one call over all stages, B = 16: bit-identical gradients.  (test_gpu_unet.py's
    test_staged_backward_equals_single_call cuts a B = 6 backward into four ranges.)"""
    from tiny_diffusion_amd._lib import check, lib

    m = _model("cond")
    g = torch.Generator().manual_seed(3)
    B = 16
    x = torch.randn(B, 1, 28, 28, generator=g).cuda()
    t = torch.randint(0, 1000, (B,), generator=g).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    d_out = torch.randn(B, 1, 28, 28, generator=g).cuda()
    _, views = m._grad_buffers(x.device)
    flat = m._grad_flat
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    _, plan, _ = m._run_forward(x, t, y, mode=0)
    m._run_backward(plan, d_out, views)
    torch.cuda.synchronize()
    want = flat.clone()
    assert want.abs().max() > 0
    m.load_state_dict(sd)   # the same BatchNorm buffers for the second forward
    flat.zero_()
    _, plan, _ = m._run_forward(x, t, y, mode=0)
    comm = torch.cuda.Stream()
    for lo, hi in ((0, 5), (5, 15)):
        m._run_backward(plan, d_out, views, lo, hi)
        comm.wait_stream(torch.cuda.current_stream())
        check(lib.tdx_unet_backward_join(plan.handle, comm.cuda_stream), "tdx_unet_backward_join")
    torch.cuda.current_stream().wait_stream(comm)
    torch.cuda.synchronize()
    assert torch.equal(flat, want)
