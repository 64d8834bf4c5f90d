"""The training timestep sampler on the MI355X (csrc/timestep.hip): the four C entries through ctypes
against the integer / fp64 restatements of tests/timestep_helpers.py, then ``TransformerTrainStep`` and ``TrainStep``
(latent MLP) under a fixed table and under the loss-second-moment resampler: the draws are the helper's from the
device's own CDF, the helper fed with ``sample_losses`` reproduces the device state, a captured step is the eager one,
a uniform table with importance weights changes nothing but ``t``, and the default step is untouched."""
import functools

import numpy as np
import pytest
import torch

import timestep_helpers as H
from oracle.weights import make_state_dict_latent, make_state_dict_transformer

pytestmark = pytest.mark.gpu

U_PROB = float(np.float32(0.001))   # uniform_prob reaches the kernel as a C float


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from tiny_diffusion_amd._lib import check, lib
    return lib, check


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _i64(v):
    return v - 2 ** 64 if v >= 2 ** 63 else v


# ------------------------------------------------------------------ tables
@functools.lru_cache(maxsize=None)
def _tables(T):
    """fp32 probability tables of length T (unnormalised), shared and never written: zero entries first, in the middle
    and last (several trailing) wherever T leaves room."""
    g = np.random.default_rng(100 + T)
    if T == 1:
        return (np.array([3.0], dtype=np.float32),)
    if T == 2:
        return tuple(np.array(p, dtype=np.float32) for p in ([0.3, 0.7], [1.0, 0.0], [0.0, 2.0]))
    p = g.random(T).astype(np.float32) + np.float32(0.01)
    q = p.copy()
    q[0] = 0
    q[T // 2] = 0
    q[-2:] = 0
    if T >= 100:
        q[:3] = 0
        q[400:421] = 0
        q[-5:] = 0
    spike = np.zeros(T, dtype=np.float32)
    spike[T // 3] = 1
    return p, q, spike, np.full(T, 1.0 / T, dtype=np.float32)


def _cdf_dev(probs, w_obj=None, importance=1):
    lib, check = _lib()
    T = probs.shape[0]
    p = _dev(probs)
    w = None if w_obj is None else _dev(w_obj)
    cdf = torch.full((T,), float("nan"), device="cuda")
    w_eff = torch.full((T,), float("nan"), device="cuda")
    check(lib.tdx_timestep_cdf(p.data_ptr(), None if w is None else w.data_ptr(), importance, cdf.data_ptr(),
                               w_eff.data_ptr(), T, _st()), "tdx_timestep_cdf")
    return cdf.cpu().numpy(), w_eff.cpu().numpy()


# ------------------------------------------------------------------ 1. tdx_timestep_cdf
@pytest.mark.parametrize("T", [1, 2, 7, 1000, 1537])
def test_cdf_against_fp64(T):
    """cdf and w_eff within 1 fp32 ulp of the sequential fp64 prefix sum (the device adds in blocks: a re-associated
    double sum moves the single fp32 rounding only at a tie), non-decreasing, exactly 1 from the last positive entry
    on, w_eff exactly 0 where p == 0.  T = 1537: seven timesteps per thread, the last threads idle."""
    g = np.random.default_rng(T)
    w_obj = (g.random(T) * 3).astype(np.float32)
    for probs in _tables(T if T != 1537 else 1000):
        if T == 1537:
            probs = np.concatenate([probs, probs[:537]])
        p64 = probs.astype(np.float64) / probs.astype(np.float64).sum()
        want = H.cdf_of(probs)
        last = int(np.flatnonzero(probs > 0)[-1])
        for w, imp in ((None, 1), (w_obj, 1), (w_obj, 0), (None, 0)):
            cdf, w_eff = _cdf_dev(probs, w, imp)
            assert H.ulp_diff(cdf, want) <= 1
            assert (cdf[last:] == 1.0).all() and (np.diff(cdf) >= 0).all() and cdf[-1] == 1.0
            assert (cdf[:last] < 1.0).all()     # (every positive entry of these tables is > 1e-5 of the sum)
            want_w = H.w_eff_of(p64, w, bool(imp))
            assert H.ulp_diff(w_eff, want_w) <= 1 and (w_eff[probs == 0] == 0).all()
            if not imp:
                assert (w_eff == want_w).all()      # copies


# ------------------------------------------------------------------ 2. tdx_timestep_draw
def _draw_dev(cdf, B, seed, offset, rng_dev=False):
    lib, check = _lib()
    c = _dev(cdf)
    t = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    u = torch.full((B,), float("nan"), device="cuda")
    if rng_dev:   # the by-value pair must then be ignored
        words = torch.tensor([_i64(seed), _i64(offset)], dtype=torch.int64).cuda()
        check(lib.tdx_timestep_draw(c.data_ptr(), cdf.shape[0], t.data_ptr(), u.data_ptr(), B, 99, 98, words.data_ptr(), _st()),
              "tdx_timestep_draw")
    else:
        check(lib.tdx_timestep_draw(c.data_ptr(), cdf.shape[0], t.data_ptr(), u.data_ptr(), B, seed, offset, None, _st()),
              "tdx_timestep_draw")
    return t.cpu().numpy(), u.cpu().numpy()


@pytest.mark.parametrize("T", [1, 2, 7, 1000])
@pytest.mark.parametrize("B", [1, 3, 64, 257])
def test_draw_is_the_helper_exactly(T, B):
    keys = [(0, 0), (1234, 5), (2 ** 64 - 3, 2 ** 32 + 7), (2 ** 63 + 11, 2 ** 40 + 1)]
    b = np.arange(B)
    for probs in _tables(T):
        cdf = H.cdf_of(probs)
        allowed = set(np.flatnonzero(probs > 0).tolist())
        for seed, offset in keys:
            u_want = H.uniform_of(seed, offset, b)
            t_want = H.draw(cdf, u_want)
            t, u = _draw_dev(cdf, B, seed, offset)
            assert u.dtype == np.float32 and (u == u_want).all() and (u < 1).all()
            assert (t == t_want).all() and set(t.tolist()) <= allowed
            t2, u2 = _draw_dev(cdf, B, seed, offset, rng_dev=True)
            assert (t2 == t).all() and (u2 == u).all()
    lib, check = _lib()     # u_out is optional
    c, t = _dev(H.cdf_of(_tables(T)[0])), torch.zeros(B, dtype=torch.int64, device="cuda")
    check(lib.tdx_timestep_draw(c.data_ptr(), T, t.data_ptr(), None, B, 1234, 5, None, _st()), "tdx_timestep_draw")
    assert (t.cpu().numpy() == H.draw(H.cdf_of(_tables(T)[0]), H.uniform_of(1234, 5, b))).all()


# ------------------------------------------------------------------ 3. tdx_mse_per_sample
@pytest.mark.parametrize("per", [3, 20, 784, 1028])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("offset", [0, 1])
def test_per_sample_loss_against_fp64(per, B, offset):
    """per 3: less than a wave; 20, 784: float4 with fewer vectors than threads; 1028: 257 vectors, thread 0 makes two
    trips.  offset 1: both pointers one float past a 16-byte boundary - the scalar path at every size.

    Bound 2^-22 per sample: the differences of two fp32 are exact in double, their squares and the <= 1028 additions of
    non-negative terms are double operations (relative error < 1030 x 2^-53 = 1.2e-13), as are the product with the
    weight and the division by per_sample; the ONE rounding to fp32 adds 2^-24.  The fp64 reference carries the same
    1e-13.  2^-24 (1 + 1e-5) < 2^-22."""
    lib, check = _lib()
    g = torch.Generator().manual_seed(per * 10 + B)
    T = 10
    a_buf = torch.randn(B * per + 1, generator=g).cuda()
    b_buf = torch.randn(B * per + 1, generator=g).cuda()
    a, b = a_buf[offset:offset + B * per], b_buf[offset:offset + B * per]
    assert a.data_ptr() % 16 == 4 * offset and b.data_ptr() % 16 == 4 * offset
    t = torch.randint(0, T, (B,), generator=g)
    w = torch.rand(T, generator=g) * 4
    w[int(t[0])] = 0.37
    sq = ((a.cpu().double() - b.cpu().double()) ** 2).view(B, per).sum(1) / per
    t_d, w_d = t.cuda(), w.cuda()
    for weights in (None, w_d):
        want = sq if weights is None else w.double()[t] * sq
        outs = []
        for _ in range(2):
            out = torch.full((B,), float("nan"), device="cuda")
            check(lib.tdx_mse_per_sample(a.data_ptr(), b.data_ptr(), t_d.data_ptr(),
                                         None if weights is None else weights.data_ptr(), out.data_ptr(), B, per, _st()),
                  "tdx_mse_per_sample")
            outs.append(out.cpu())
        rel = ((outs[0].double() - want).abs() / want).max().item()
        print(f"per-sample loss per={per} B={B} offset={offset} weights={weights is not None}: max rel {rel:.3g}")
        assert rel <= 2.0 ** -22
        assert torch.equal(outs[0], outs[1])      # bit-reproducible
    # without weights t may be NULL
    out = torch.zeros(B, device="cuda")
    check(lib.tdx_mse_per_sample(a.data_ptr(), b.data_ptr(), None, None, out.data_ptr(), B, per, _st()), "tdx_mse_per_sample")
    assert ((out.cpu().double() - sq).abs() / sq).max().item() <= 2.0 ** -22


# ------------------------------------------------------------------ 4. tdx_timestep_history_update
class _Resampler:
    """The device state of one resampler beside the helper's."""

    def __init__(self, T, Hn, w_obj=None, history=None, counts=None):
        self.T, self.H = T, Hn
        self.ref = H.LossSecondMoment(T, Hn, U_PROB)
        if history is not None:
            self.ref.history[:], self.ref.counts[:] = history, counts
        self.history, self.counts = _dev(self.ref.history), _dev(self.ref.counts)
        self.w_obj = w_obj
        self.w = None if w_obj is None else _dev(w_obj)
        self.cdf = torch.full((T,), float("nan"), device="cuda")
        self.w_eff = torch.full((T,), float("nan"), device="cuda")

    def update(self, t, losses):
        lib, check = _lib()
        B = len(t)
        t_d = None if B == 0 else _dev(np.asarray(t, dtype=np.int64))
        l_d = None if B == 0 else _dev(np.asarray(losses, dtype=np.float32))
        check(lib.tdx_timestep_history_update(None if B == 0 else t_d.data_ptr(), None if B == 0 else l_d.data_ptr(), B,
                                              self.history.data_ptr(), self.counts.data_ptr(), self.H, U_PROB,
                                              None if self.w is None else self.w.data_ptr(), self.cdf.data_ptr(),
                                              self.w_eff.data_ptr(), self.T, _st()), "tdx_timestep_history_update")
        self.ref.update(t, losses)

    def check(self, what):
        hist, counts = self.ref.state()
        assert (self.counts.cpu().numpy() == counts).all(), what
        assert (self.history.cpu().numpy() == hist).all(), what          # copies of fp32 inputs, oldest first
        cdf, w_eff = self.cdf.cpu().numpy(), self.w_eff.cpu().numpy()
        want_cdf, want_w = self.ref.tables(self.w_obj)
        assert cdf[-1] == 1.0 and (np.diff(cdf) >= 0).all(), what
        if self.ref.warmed_up():
            assert H.ulp_diff(cdf, want_cdf) <= 1 and H.ulp_diff(w_eff, want_w) <= 1, what
        else:   # fl((k + 1) / T) and w_obj exactly
            assert (cdf == want_cdf).all() and (w_eff == want_w).all(), what


# duplicates within a batch, every row wraps at least once (timestep 1 takes four losses in update 5: more than H in
# one batch), the warm-up ends with the fourth update
UPDATES = [[0, 0, 1, 2], [3, 4, 4, 1], [2, 2, 3, 3], [0, 1, 4, 0], [1, 1, 1, 1], [2, 3, 4, 2], [3, 3, 4, 4], [0, 2, 3, 4]]


@pytest.mark.parametrize("weighted", [False, True])
def test_history_update_small_hand_chosen(weighted):
    g = np.random.default_rng(7)
    w_obj = (g.random(5) * 2 + 0.1).astype(np.float32) if weighted else None
    r = _Resampler(5, 3, w_obj)
    r.update([], [])        # B == 0: the first table from the empty state
    r.check("empty")
    for k, t in enumerate(UPDATES):
        r.update(t, (g.random(4) * 3 + 0.01).astype(np.float32))
        r.check(f"update {k + 1}")
        assert r.ref.warmed_up() == (k >= 3)
    assert (r.ref.counts == 3).all()
    # B == 0 rebuilds the table for another objective and leaves the state alone
    r.w_obj = (g.random(5) + 0.5).astype(np.float32)
    r.w = _dev(r.w_obj)
    r.update([], [])
    r.check("rebuild")
    # all-zero losses: the uniform probabilities, not a division by zero
    z = _Resampler(5, 3, None, np.zeros((5, 3), dtype=np.float32), np.full(5, 3, dtype=np.int32))
    z.update([], [])
    assert torch.isfinite(z.cdf).all() and H.ulp_diff(z.cdf.cpu().numpy(), H.cdf_of(np.full(5, 0.2))) <= 1
    assert H.ulp_diff(z.w_eff.cpu().numpy(), np.ones(5, dtype=np.float32)) <= 1


@pytest.mark.parametrize("warm", [True, False])
def test_history_update_T1000(warm):
    """T = 1000, H = 10, B = 256 from a seeded state: strided loops, T no multiple of the block, the batch in one piece
    of 256; then B = 300 (two pieces) and B = 1.  ``warm=False``: some rows are short, so the table stays uniform."""
    g = np.random.default_rng(1000 + warm)
    T, Hn = 1000, 10
    counts = np.full(T, Hn, dtype=np.int32) if warm else g.integers(0, Hn + 1, T).astype(np.int32)
    if not warm:
        counts[[0, 255, 256, 999]] = [0, Hn, 3, Hn - 1]     # stay short over the 557 samples below
    history = (g.random((T, Hn)) * 2 + 1e-3).astype(np.float32)
    history[np.arange(Hn)[None, :] >= counts[:, None]] = 0
    w_obj = (g.random(T) * 2 + 0.1).astype(np.float32)
    r = _Resampler(T, Hn, w_obj, history, counts)
    for B in (256, 300, 1):
        t = g.integers(0, T, B)
        if B > 1:
            t[:6] = [999, 999, 0, 256, 999, 512]      # duplicates across the strided owners, the last timestep
            if not warm:
                t[t == 0] = 1
                t[t == 256] = 257
        r.update(t, (g.random(B) * 3 + 1e-3).astype(np.float32))
        r.check(f"B={B}")
        assert r.ref.warmed_up() == warm


def test_history_update_largest_T():
    """T = 4096, the largest the entry takes (its per-timestep moments fill the LDS array), H = 2, B = 257: two pieces,
    the second of one sample that repeats a timestep of the first."""
    g = np.random.default_rng(4096)
    T, Hn = 4096, 2
    r = _Resampler(T, Hn, None, (g.random((T, Hn)) + 0.1).astype(np.float32), np.full(T, Hn, dtype=np.int32))
    t = g.integers(0, T, 257)
    t[:4] = [4095, 4095, 4095, 0]
    t[-1] = 4095
    r.update(t, (g.random(257) + 0.1).astype(np.float32))
    r.check("T=4096")
    lib, _ = _lib()
    one = r.cdf.data_ptr()
    assert lib.tdx_timestep_history_update(one, one, 1, one, one, Hn, 0.0, None, one, one, 4097, _st()) == -2


# ------------------------------------------------------------------ 5. the steps
T_S, B_S = 8, 4
FILL = [[0, 1, 2, 3], [4, 5, 6, 7]]


def _transformer(dropout=0.0):
    from tiny_diffusion_amd.diffusion_transformer import NoiseModel

    torch.manual_seed(0)
    return NoiseModel(time_dim=64, num_layers=1, dropout=dropout).cuda().train()


def _latent():
    from tiny_diffusion_amd.latent_diffusion import NoiseModel

    m = NoiseModel()
    m.load_state_dict(make_state_dict_latent(0), strict=True)
    return m.cuda().train()


def _step(kind, **kw):
    from tiny_diffusion_amd.diffusion_transformer import TransformerTrainStep
    from tiny_diffusion_amd.schedule import ForwardProcess
    from tiny_diffusion_amd.train import TrainStep

    fp = ForwardProcess(num_timesteps=T_S)
    if kind == "transformer":
        return TransformerTrainStep(_transformer(), fp, lr=1e-3, **kw)
    return TrainStep(_latent(), fp, lr=1e-3, **kw)


@functools.lru_cache(maxsize=None)
def _batches(n):
    """(z_0, y, noise) of n steps on the CPU, shared and never written."""
    g = torch.Generator().manual_seed(42)
    return [(torch.randn(B_S, 20, generator=g), torch.randint(0, 10, (B_S,), generator=g), torch.randn(B_S, 20, generator=g))
            for _ in range(n)]


def _objective_table(step):
    return None if step._w_table is None else step._w_table.cpu().numpy()


def _run_checked(step, n_fill_rounds, n_drawn, Hn, seed, noise=True):
    """Explicit ``t`` that gives every timestep ``Hn`` losses, then drawn steps; every step checked against the helper:
    the draw from the device's own CDF read back before the step, the state from ``sample_losses``, the next tables to
    1 ulp, the returned loss against mean_b(w_eff[t_b] mse_b) in fp64 (1e-6: tests/test_gpu_objective.py's bound for the
    weighted loss).  Returns the timesteps seen."""
    ref = H.LossSecondMoment(T_S, Hn, U_PROB)
    adaptive = step.timestep_sampler == "loss_second_moment"
    w_obj = _objective_table(step)
    b = np.arange(B_S)
    seen = []
    plan = [FILL[k % 2] for k in range(n_fill_rounds)] + [None] * n_drawn
    for k, ((z0, y, eps), t_given) in enumerate(zip(_batches(len(plan)), plan)):
        cdf = step._ts_cdf.cpu().numpy()
        w_eff = step._w_eff.cpu().numpy()
        offset = step.step_count
        t_arg = None if t_given is None else torch.tensor(t_given).cuda()
        loss = step.step(z0.cuda(), y.cuda(), t=t_arg, noise=eps.cuda() if noise else None)
        t = step.last_t.cpu().numpy()
        if t_given is None:
            assert (t == H.draw(cdf, H.uniform_of(seed, offset, b))).all(), k
        else:
            assert (t == np.asarray(t_given)).all(), k
        seen.append(t.copy())
        sl = step.sample_losses.cpu().numpy()
        assert sl.shape == (B_S,) and np.isfinite(sl).all() and (sl > 0).all()
        # the loss the step returned: the importance / objective weights of ITS timesteps, from the table before the step
        w_used = step._loss_table()
        mse = sl.astype(np.float64) / (1.0 if w_obj is None else w_obj[t].astype(np.float64))
        want = float(np.mean((1.0 if w_used is None else w_eff[t].astype(np.float64)) * mse))
        rel = abs(float(loss) - want) / want
        print(f"step {k} t={t.tolist()} loss {float(loss):.8g} vs fp64 {want:.8g}: rel {rel:.2e}")
        assert rel < 1e-6, (k, rel)
        if adaptive:
            ref.update(t, sl)
            state = step.timestep_sampler_state()
            hist, counts = ref.state()
            assert (state["counts"].numpy() == counts).all() and (state["history"].numpy() == hist).all(), k
            assert state["history"].shape == (T_S, Hn) and state["counts"].dtype == torch.int32
            want_cdf, want_w = ref.tables(w_obj)
            got_cdf, got_w = step._ts_cdf.cpu().numpy(), step._w_eff.cpu().numpy()
            if ref.warmed_up():
                assert H.ulp_diff(got_cdf, want_cdf) <= 1 and H.ulp_diff(got_w, want_w) <= 1, k
            else:
                assert (got_cdf == want_cdf).all() and (got_w == want_w).all(), k
            assert ref.warmed_up() == (k + 1 >= n_fill_rounds)
    return seen


@pytest.mark.parametrize("kind", ["transformer", "latent"])
def test_adaptive_steps_against_the_helper(kind):
    """Four explicit steps fill every timestep twice (the end of the warm-up does not depend on a seed), six drawn ones
    follow; the transformer under the plain objective, the latent MLP under v-prediction with min-SNR weights."""
    kw = {} if kind == "transformer" else dict(prediction="v", loss_weighting="min_snr")
    step = _step(kind, timestep_sampler="loss_second_moment", history_per_term=2, timestep_seed=77, **kw)
    assert step.importance_weights is True and step.uniform_prob == 0.001
    assert (step._loss_table() is step._w_eff) and step._w_eff is not step._w_table
    if kind == "latent":    # the diffusion's cached table is shared by every step on the device: never written
        before = step._w_table.clone()
    seen = _run_checked(step, 4, 6, 2, 77)
    assert len({tuple(t) for t in seen[4:]}) > 1       # fresh timesteps every step
    if kind == "latent":
        assert torch.equal(step._w_table, before)
        assert step._w_table is step.diffusion.loss_weight_table(step.device, "v", "min_snr", 5.0)
    # a checkpoint: the state into a fresh step gives the same tables, bit for bit (same entry, same inputs)
    other = _step(kind, timestep_sampler="loss_second_moment", history_per_term=2, **kw)
    assert (other._ts_cdf.cpu().numpy() == H.LossSecondMoment(T_S, 2).tables()[0]).all()
    other.load_timestep_sampler_state(step.timestep_sampler_state())
    assert torch.equal(other._ts_cdf, step._ts_cdf) and torch.equal(other._w_eff, step._w_eff)
    assert torch.equal(other.timestep_sampler_state()["history"], step.timestep_sampler_state()["history"])
    # set_objective rebuilds the step's weights from the new objective's table; the history stays
    ref = H.LossSecondMoment(T_S, 2, U_PROB)
    st = step.timestep_sampler_state()
    ref.history[:], ref.counts[:] = st["history"].numpy(), st["counts"].numpy()
    step.set_objective(prediction="eps", loss_weighting=torch.linspace(0.5, 2.0, T_S))
    assert torch.equal(step._w_table.cpu(), torch.linspace(0.5, 2.0, T_S))
    want_cdf, want_w = ref.tables(step._w_table.cpu().numpy())
    assert H.ulp_diff(step._ts_cdf.cpu().numpy(), want_cdf) <= 1 and H.ulp_diff(step._w_eff.cpu().numpy(), want_w) <= 1
    assert torch.equal(step.timestep_sampler_state()["history"], st["history"])


@pytest.mark.parametrize("kind", ["transformer", "latent"])
def test_fixed_table_steps(kind):
    """A logit-normal table: the draws are the helper's, ``sample_losses`` is public, the loss is unweighted without
    importance weights and weighted by 1 / (T p) with them; the cuda generator is not consumed for ``t``."""
    from tiny_diffusion_amd.schedule import logit_normal_timestep_probs

    probs = logit_normal_timestep_probs(T_S)
    for imp in (None, True):
        step = _step(kind, timestep_sampler=probs, importance_weights=imp, timestep_seed=5)
        assert step.timestep_sampler == "table" and step.importance_weights is bool(imp)
        assert (step._loss_table() is None) == (not imp)
        p32 = probs.to(torch.float32).numpy()
        assert H.ulp_diff(step._ts_cdf.cpu().numpy(), H.cdf_of(p32)) <= 1
        p64 = p32.astype(np.float64) / p32.astype(np.float64).sum()
        assert H.ulp_diff(step._w_eff.cpu().numpy(), H.w_eff_of(p64, None, bool(imp))) <= 1
        rng = torch.cuda.get_rng_state()
        _run_checked(step, 0, 4, 1, 5)
        assert torch.equal(torch.cuda.get_rng_state(), rng)
        with pytest.raises(RuntimeError):
            step.timestep_sampler_state()


def test_captured_transformer_step_is_the_eager_step():
    """use_graph against eager with the same seeds and supplied noise, dropout 0: three steps with explicit ``t`` (the
    eager one, the capture, a replay; history_per_term = 1, so the warm-up ends with the second) and five drawn ones."""
    steps = {}
    for use_graph in (False, True):
        steps[use_graph] = _step("transformer", timestep_sampler="loss_second_moment", history_per_term=1,
                                 timestep_seed=2 ** 63 + 5, use_graph=use_graph)
    plan = [FILL[0], FILL[1], [0, 0, 7, 7]] + [None] * 5
    for k, ((z0, y, eps), t_given) in enumerate(zip(_batches(len(plan)), plan)):
        out = {}
        for use_graph, step in steps.items():
            t_arg = None if t_given is None else torch.tensor(t_given).cuda()
            loss = step.step(z0.cuda(), y.cuda(), t=t_arg, noise=eps.cuda())
            out[use_graph] = (loss.clone(), step.last_t.clone(), step.sample_losses.clone(), step._ts_cdf.clone(),
                              step._w_eff.clone())
        for a, b in zip(out[False], out[True]):
            assert torch.equal(a, b), k
        sa, sb = (s.timestep_sampler_state() for s in steps.values())
        assert torch.equal(sa["history"], sb["history"]) and torch.equal(sa["counts"], sb["counts"]), k
        assert torch.equal(steps[False].flat_param, steps[True].flat_param), k
    assert steps[True]._graph is not None and bool((sa["counts"] == 1).all()) and steps[True].step_count == len(plan)


def test_captured_latent_step_draws_and_learns_like_the_helper():
    """``TrainStep(use_graph=True)`` draws inside the graph from the device words the host refreshes before each replay:
    the eager step, the capture and three replays all see the helper's timesteps and leave the helper's state.  (Its
    noise is torch's, inside the graph: nothing here compares against an eager run's parameters.)"""
    step = _step("latent", timestep_sampler="loss_second_moment", history_per_term=2, timestep_seed=9, use_graph=True)
    _run_checked(step, 4, 5, 2, 9, noise=False)
    assert step._graph is not None and step.step_count == 9


@pytest.mark.parametrize("kind", ["transformer", "latent"])
def test_uniform_table_with_importance_weights_changes_only_t(kind):
    """A uniform table under importance weights has w_eff == 1 exactly, and the weighted loss entries with a table of
    ones are the unweighted ones bit for bit: replaying the sampler step's ``t`` and noise through a default step gives
    its losses and parameters."""
    a = _step(kind, timestep_sampler=torch.full((T_S,), 1.0 / T_S), importance_weights=True, timestep_seed=3)
    b = _step(kind)
    assert a._loss_table() is a._w_eff and bool((a._w_eff == 1.0).all()) and b._loss_table() is None
    assert torch.equal(a.flat_param, b.flat_param)
    for k, (z0, y, eps) in enumerate(_batches(4)):
        la = a.step(z0.cuda(), y.cuda(), noise=eps.cuda()).clone()
        lb = b.step(z0.cuda(), y.cuda(), t=a.last_t.clone(), noise=eps.cuda()).clone()
        assert torch.equal(la, lb), k
        assert torch.equal(a.flat_param, b.flat_param), k
    assert b.sample_losses is None and b.last_t is None


@pytest.mark.parametrize("kind", ["transformer", "latent"])
def test_default_step_is_untouched(kind, monkeypatch):
    """No keyword: no sampler, no buffer, no launch of the new entries, ``torch.randint`` as before."""
    from tiny_diffusion_amd import _flat_step

    step = _step(kind)
    assert step.timestep_sampler is None and step.sample_losses is None and step.last_t is None
    assert step._ts_cdf is None and step._w_eff is None and step._ts_history is None and step._ts_counts is None
    assert step.importance_weights is False

    class Guard:
        def __getattr__(self, name):
            assert name not in ("tdx_timestep_cdf", "tdx_timestep_draw", "tdx_mse_per_sample",
                                "tdx_timestep_history_update"), name
            return getattr(_flat_step._lib.lib, name)

    monkeypatch.setattr(_flat_step, "lib", Guard())
    z0, y, eps = _batches(1)[0]
    rng = torch.cuda.get_rng_state()
    step.step(z0.cuda(), y.cuda(), noise=eps.cuda())
    assert not torch.equal(torch.cuda.get_rng_state(), rng)      # randint drew t
    assert step.sample_losses is None and step.last_t is None and step._sl == {}
    with pytest.raises(RuntimeError):
        step.timestep_sampler_state()
