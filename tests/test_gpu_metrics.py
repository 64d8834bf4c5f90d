"""The pairwise metric kernels (csrc/metrics.hip) and tiny_diffusion_amd/metrics.py on the device,
against the fp64 references and the derived bounds of tests/metrics_helpers.py.

Sizes: 133 real and 70 generated rows (no multiple of any tile), one case of 300 rows under col_chunks 1, 2 and 5 (three
128-row tiles: the merge launch runs with a ragged last chunk), d = 1 (one K step, zero pad), 20 (the VAE latent), 33 (an
odd K tail past one 32-wide slice) and 784 (MNIST pixels, 25 slices)."""
import functools
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_helpers as H  # noqa: E402

from tiny_diffusion_amd import _lib, metrics as M  # noqa: E402
from tiny_diffusion_amd._lib import lib  # noqa: E402

TDX_E_BADARG = -1
DIMS = (1, 20, 33, 784)
NEW = ("tdx_pair_scratch_bytes", "tdx_pair_gram", "tdx_pair_kth_dist2", "tdx_pair_member", "tdx_pair_poly_rowsum")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # a copy: the cached sets are read-only


def _st():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _sets(seed, d, shift, n_real=133, n_gen=70):
    """The centred real and generated set (numpy fp32, read-only) of one case."""
    x, y = H.centre_ref(*H.inputs(seed, n_real, n_gen, d, shift))
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def _radii(seed, d, shift, k=3):
    """fp64 radii and their bounds of both sets, and the device radii of both sets."""
    x, y = _sets(seed, d, shift)
    ref = (H.kth_dist2_ref(x, x, k, True), H.kth_dist2_ref(y, y, k, True))
    bound = (H.kth_dist2_bound(x, x, True), H.kth_dist2_bound(y, y, True))
    dev = (M.pair_kth_dist2(_dev(x), _dev(x), k, True), M.pair_kth_dist2(_dev(y), _dev(y), k, True))
    return ref, bound, dev


# ------------------------------------------------------------------ 1. tdx_pair_gram
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("na,nb", [(1, 1), (31, 33), (70, 133)])
def test_gram_per_element(na, nb, d, seed):
    x, y = _sets(seed, d, 0.3)
    a, b = y[:na], x[:nb]
    g = M.pair_gram(_dev(a), _dev(b)).cpu().numpy()
    err, bound = np.abs(g - H.gram_ref(a, b)), H.gram_bound(a, b)
    print(f"gram ({na},{nb}) d={d}: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert g.shape == (na, nb) and (err <= bound).all()


def test_gram_is_not_symmetric_in_its_arguments_and_leaves_its_neighbours_alone():
    """a_i . b_j lands at [i, j] (an asymmetric pair of sets), and nothing is written past (na, nb)."""
    x, y = _sets(0, 33, 0.3)
    a, b = _dev(y[:31]), _dev(x[:40])
    out = torch.full((31 * 40 + 64,), -7.0, device="cuda")
    _lib.check(lib.tdx_pair_gram(a.data_ptr(), b.data_ptr(), 31, 40, 33, out.data_ptr(), _st()))
    g = out[:31 * 40].reshape(31, 40).cpu().numpy()
    assert (np.abs(g - H.gram_ref(y[:31], x[:40])) <= H.gram_bound(y[:31], x[:40])).all()
    assert (out[31 * 40:] == -7.0).all()


# ------------------------------------------------------------------ 2. tdx_pair_kth_dist2
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("k", [1, 3, 8])
def test_kth_dist2_within_bound(k, d, seed):
    x, y = _sets(seed, d, 0.3)
    for a, b, excl in ((x, x, True), (y, y, True), (y, x, False), (x, y, False)):
        got = M.pair_kth_dist2(_dev(a), _dev(b), k, excl).cpu().numpy().astype(np.float64)
        err, bound = np.abs(got - H.kth_dist2_ref(a, b, k, excl)), H.kth_dist2_bound(a, b, excl)
        print(f"kth k={k} d={d} {a.shape[0]}x{b.shape[0]} excl={excl}: max err / bound {np.max(err / bound):.3f}")
        assert (err <= bound).all()


def test_kth_dist2_excludes_by_index_not_by_distance():
    """Rows 5 and 90 are the same point, and so are rows 17, 18 and 131: their nearest other row is at distance
    exactly 0 (the norm and the Gram chain of identical rows are the same bits), which an exclusion by distance
    (d2 > 0) would skip.  Without the exclusion every row finds itself at 0."""
    x = np.array(_sets(0, 33, 0.0)[0])
    x[90] = x[5]
    x[18] = x[17]
    x[131] = x[17]
    xd = _dev(x)
    r1 = M.pair_kth_dist2(xd, xd, 1, True).cpu().numpy()
    dup = [5, 90, 17, 18, 131]
    rest = np.setdiff1d(np.arange(133), dup)
    assert (r1[dup] == 0.0).all()
    assert (r1[rest] > 0.0).all()
    assert (np.abs(r1 - H.kth_dist2_ref(x, x, 1, True)) <= H.kth_dist2_bound(x, x, True)).all()
    r2 = M.pair_kth_dist2(xd, xd, 2, True).cpu().numpy()
    assert (r2[[17, 18, 131]] == 0.0).all() and (r2[[5, 90]] > 0.0).all()
    assert (M.pair_kth_dist2(xd, xd, 1, False) == 0.0).all()


@pytest.mark.parametrize("d", [20, 784])
def test_kth_dist2_and_member_are_the_same_bits_for_every_chunking(d):
    x, _ = H.centre_ref(*H.inputs(0, 300, 70, d, 0.3))
    y = H.inputs(1, 290, 70, d, 0.3)[0] + np.float32(0.3)
    xd, yd = _dev(x), _dev(y)
    base = M.pair_kth_dist2(xd, xd, 3, True, col_chunks=1)
    assert (np.abs(base.cpu().numpy() - H.kth_dist2_ref(x, x, 3, True)) <= H.kth_dist2_bound(x, x, True)).all()
    flags = M.pair_member(yd, xd, base, col_chunks=1)
    assert 0 < int(flags.sum()) < 290
    for chunks in (1, 2, 5, 0):
        assert torch.equal(M.pair_kth_dist2(xd, xd, 3, True, col_chunks=chunks), base), chunks
        assert torch.equal(M.pair_kth_dist2(yd, xd, 8, False, col_chunks=chunks),
                           M.pair_kth_dist2(yd, xd, 8, False, col_chunks=1)), chunks
        assert torch.equal(M.pair_member(yd, xd, base, col_chunks=chunks), flags), chunks


def test_kth_dist2_refuses_bad_k_and_writes_nothing():
    x = _dev(_sets(0, 20, 0.0)[0])
    out = torch.full((133,), -7.0, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.float64, device="cuda")

    def call(nb, k, excl, chunks=0):
        return lib.tdx_pair_kth_dist2(x.data_ptr(), x.data_ptr(), 133, nb, 20, k, excl, chunks, out.data_ptr(),
                                      ws.data_ptr(), ws.numel() * 8, _st())

    assert call(133, 9, 1) == TDX_E_BADARG and call(133, 0, 1) == TDX_E_BADARG
    assert call(3, 3, 1) == TDX_E_BADARG            # nb = k with the diagonal excluded
    assert call(2, 3, 0) == TDX_E_BADARG and call(133, 3, 1, -1) == TDX_E_BADARG
    assert lib.tdx_pair_kth_dist2(x.data_ptr(), None, 133, 133, 20, 3, 1, 0, out.data_ptr(), ws.data_ptr(),
                                  ws.numel() * 8, _st()) == TDX_E_BADARG
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert call(3, 3, 0) == 0 and call(4, 3, 1) == 0     # the same calls, valid, do write
    torch.cuda.synchronize()
    assert (out >= 0.0).all()


# ------------------------------------------------------------------ 3. tdx_pair_member
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shift", [0.0, 0.3])
def test_member_on_every_decidable_query(shift, d, seed):
    x, y = _sets(seed, d, shift)
    ref, bound, dev = _radii(seed, d, shift)
    for q, c, side in ((y, x, 0), (x, y, 1)):
        flags = M.pair_member(_dev(q), _dev(c), dev[side]).cpu().numpy()
        sure_in, sure_out = H.member_decidable(q, c, ref[side], bound[side])
        left_out = int((~(sure_in | sure_out)).sum())
        print(f"member d={d} shift={shift} {q.shape[0]} queries: {int(flags.sum())} in, {left_out} left out")
        assert set(np.unique(flags)) <= {0, 1}
        assert left_out <= 0.02 * q.shape[0]
        assert (flags[sure_in] == 1).all() and (flags[sure_out] == 0).all()


@pytest.mark.parametrize("d", [20, 784])
def test_member_detects_the_radii_of_the_wrong_set(d):
    """The radius belongs to the candidate.  The same call with the radii of the QUERY set in place of the candidates'
    (133 real queries against 133 shifted candidates, so both radius vectors fit) disagrees with the reference on
    decidable queries, while the right call agrees on all of them."""
    x = _sets(0, d, 0.3)[0]
    c = H.inputs(1, 133, 70, d, 0.3)[0] * np.float32(0.6) + np.float32(0.3)   # a tighter cloud: smaller radii
    r_c, r_x = H.kth_dist2_ref(c, c, 3, True), H.kth_dist2_ref(x, x, 3, True)
    sure_in, sure_out = H.member_decidable(x, c, r_c, H.kth_dist2_bound(c, c, True))
    xd, cd = _dev(x), _dev(c)
    right = M.pair_member(xd, cd, M.pair_kth_dist2(cd, cd, 3, True)).cpu().numpy()
    wrong = M.pair_member(xd, cd, M.pair_kth_dist2(xd, xd, 3, True)).cpu().numpy()
    assert (right[sure_in] == 1).all() and (right[sure_out] == 0).all()
    assert (~(sure_in | sure_out)).sum() <= 0.02 * 133
    assert (wrong[sure_out] == 1).any() or (wrong[sure_in] == 0).any()
    assert not np.array_equal(H.member_ref(x, c, r_x), H.member_ref(x, c, r_c))


# ------------------------------------------------------------------ 4. tdx_pair_poly_rowsum
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("d", DIMS)
def test_poly_rowsum_within_bound(d, seed):
    x, y = _sets(seed, d, 0.3)
    g = np.float32(1.0 / d)
    for a, b, excl in ((x, x, True), (x, x, False), (y, x, False), (x, y, True)):
        ad, bd = _dev(a), _dev(b)
        got = M.pair_poly_rowsum(ad, bd, float(g), 1.0, excl)
        assert got.dtype == torch.float64 and got.shape == (a.shape[0],)
        assert torch.equal(M.pair_poly_rowsum(ad, bd, float(g), 1.0, excl), got)
        err = np.abs(got.cpu().numpy() - H.poly_rowsum_ref(a, b, g, 1.0, excl))
        bound = H.poly_rowsum_bound(a, b, g, 1.0, excl)
        print(f"poly d={d} {a.shape[0]}x{b.shape[0]} excl={excl}: max err / bound {np.max(err / bound):.3f}")
        assert (err <= bound).all()


def test_poly_rowsum_over_chunks_and_other_constants():
    x = H.inputs(0, 300, 70, 33, 0.0)[0]
    xd = _dev(x)
    ref, bound = H.poly_rowsum_ref(x, x, -0.07, 0.5, True), H.poly_rowsum_bound(x, x, -0.07, 0.5, True)
    for chunks in (1, 2, 5):
        got = M.pair_poly_rowsum(xd, xd, -0.07, 0.5, True, col_chunks=chunks).cpu().numpy()
        assert (np.abs(got - ref) <= bound).all(), chunks


# ------------------------------------------------------------------ 5. the metrics end to end
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("d", [20, 33, 784])
@pytest.mark.parametrize("shift", [0.0, 0.3])
def test_precision_recall_equals_the_reference(shift, d, seed):
    real, gen = H.inputs(seed, 133, 70, d, shift)
    pr = M.precision_recall(_dev(real), _dev(gen), k=3)
    xd, yd = M.centre_on(_dev(real), _dev(gen))
    x, y = H.centre_ref(real, gen)
    assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(yd.cpu().numpy(), y)
    p, r, out_p, out_r = H.precision_recall_ref(x, y, 3)
    assert out_p == 0 and out_r == 0
    assert pr.precision == p and pr.recall == r, (pr, p, r)
    assert 0.0 < p < 1.0 and 0.0 < r < 1.0


@pytest.mark.parametrize("d", DIMS)
def test_kernel_distance_within_the_propagated_bound(d):
    real, gen = H.inputs(0, 133, 70, d, 0.3)
    kd = M.kernel_distance(_dev(real), _dev(gen))
    ref, bound = H.kid_ref(real, gen)
    print(f"KID d={d}: {kd.kid:.6e} ref {ref:.6e} bound {bound:.2e}")
    assert isinstance(kd, M.KernelDistance) and kd.std == 0.0
    assert abs(kd.kid - ref) <= bound
    sub = M.kernel_distance(_dev(real), _dev(gen), subset_size=32, n_subsets=4, seed=3)
    vals = [H.kid_ref(real[ia], gen[ib]) for ia, ib in M.kid_subsets(133, 70, 32, 4, 3)]
    assert abs(sub.kid - np.mean([v for v, _ in vals])) <= max(b for _, b in vals)
    assert abs(sub.std - np.std([v for v, _ in vals])) <= 2 * max(b for _, b in vals)
    assert sub == M.kernel_distance(_dev(real), _dev(gen), subset_size=32, n_subsets=4, seed=3)


@pytest.mark.parametrize("d", [20, 33, 784])
def test_feature_stats_and_frechet_distance(d):
    real, gen = H.inputs(1, 133, 70, d, 0.3)
    moments = []
    for f, cuts in ((real, (0, 50, 51, 133)), (gen, (0, 7, 40, 70))):
        batches = [f[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        st = M.FeatureStats()
        for b in batches:
            st.update(_dev(b))
        n, mean, cov, mean_bound, cov_bound = H.stats_ref(batches, st.pivot.cpu().numpy())
        assert st.count == n == f.shape[0]
        assert st.mean().dtype == torch.float64 and st.cov().dtype == torch.float64 and not st.cov().is_cuda
        assert (np.abs(st.mean().numpy() - mean) <= mean_bound).all()
        err = np.abs(st.cov().numpy() - cov)
        print(f"cov d={d} n={n}: max err / bound {np.max(err / cov_bound):.3f}")
        assert (err <= cov_bound).all()
        # and the restated moments are those of the raw features up to the one rounding of f - pivot
        raw = np.cov(f.astype(np.float64), rowvar=False).reshape(d, d)
        assert np.abs(cov - raw).max() <= 8 * H.U * np.abs(raw).max() * 4
        moments.append((st, mean, cov, mean_bound, cov_bound))
    (sa, mu_a, cov_a, mb_a, cb_a), (sb, mu_b, cov_b, mb_b, cb_b) = moments
    fd = M.frechet_distance(sa, sb)
    ref = H.frechet_ref(mu_a, cov_a, mu_b, cov_b)
    bound = H.frechet_bound(mu_a, cov_a, mu_b, cov_b, mb_a, cb_a, mb_b, cb_b)
    print(f"FD d={d}: {fd:.9f} ref {ref:.9f} bound {bound:.2e}")
    assert abs(fd - ref) <= bound
    assert abs(M.frechet_distance(sa, sa)) <= H.frechet_bound(mu_a, cov_a, mu_a, cov_a, mb_a, cb_a, mb_a, cb_a)


def test_feature_stats_chunks_its_rows(monkeypatch):
    """A batch longer than GRAM_ROWS goes through several Gram calls and gives the moments of the whole batch."""
    monkeypatch.setattr(M, "GRAM_ROWS", 50)
    real = H.inputs(0, 133, 70, 20, 0.0)[0]
    calls = []
    real_gram = lib.tdx_pair_gram
    monkeypatch.setattr(lib, "tdx_pair_gram", lambda *a: (calls.append(a[4]), real_gram(*a))[1])
    st = M.FeatureStats().update(_dev(real))
    assert calls == [50, 50, 33]
    _, mean, cov, mean_bound, cov_bound = H.stats_ref([real], st.pivot.cpu().numpy(), chunk=50)
    assert (np.abs(st.cov().numpy() - cov) <= cov_bound).all() and (np.abs(st.mean().numpy() - mean) <= mean_bound).all()


def test_evaluate_samples_with_a_vae_extractor():
    from tiny_diffusion_amd.vae import VAE, VAEConfig

    torch.manual_seed(0)
    vae = VAE(VAEConfig()).cuda().eval()
    g = torch.Generator().manual_seed(1)
    real = torch.rand(133, 1, 28, 28, generator=g).cuda()
    gen = (torch.rand(70, 1, 28, 28, generator=g) * 0.8 + 0.1).cuda()
    q = M.evaluate_samples(real, gen, extractor=vae, k=3)
    assert isinstance(q, M.SampleQuality)
    with torch.no_grad():
        fr = vae.encode(real.reshape(133, 784))[0]
        fg = vae.encode(gen.reshape(70, 784))[0]
    assert torch.equal(M.features(real, vae), fr) and fr.shape == (133, 20)
    assert torch.equal(M.features(real), real.reshape(133, 784))
    assert torch.equal(M.features(real, lambda t: t[:, :, ::2]), real[:, :, ::2].reshape(133, 392))
    fr, fg = fr.cpu().numpy(), fg.cpu().numpy()
    # the reference metrics from the same fp32 features
    kid, kid_bound = H.kid_ref(fr, fg)
    assert abs(q.kid - kid) <= kid_bound
    x, y = H.centre_ref(fr, fg)
    p, r, out_p, out_r = H.precision_recall_ref(x, y, 3)
    print(f"VAE features: P {q.precision:.4f} (ref {p:.4f}, {out_p} left out) R {q.recall:.4f} (ref {r:.4f}, {out_r})")
    assert abs(q.precision - p) <= out_p / 70 and abs(q.recall - r) <= out_r / 133
    parts = []
    for f in (fr, fg):
        pivot = f.astype(np.float64).mean(axis=0).astype(np.float32)     # FeatureStats' pivot: one update
        parts.append(H.stats_ref([f], pivot)[1:])
    (mu_a, cov_a, mb_a, cb_a), (mu_b, cov_b, mb_b, cb_b) = parts
    fd_bound = H.frechet_bound(mu_a, cov_a, mu_b, cov_b, mb_a, cb_a, mb_b, cb_b)
    print(f"VAE features: FD {q.fd:.6e} ref {H.frechet_ref(mu_a, cov_a, mu_b, cov_b):.6e} bound {fd_bound:.2e}")
    assert abs(q.fd - H.frechet_ref(mu_a, cov_a, mu_b, cov_b)) <= fd_bound


# ------------------------------------------------------------------ 6. nothing else moved
def test_training_and_sampling_call_none_of_the_new_entries(monkeypatch):
    from oracle.weights import make_state_dict
    from tiny_diffusion_amd.diffusion import ForwardProcess, NoiseModel, sample
    from tiny_diffusion_amd.train import TrainStep

    calls = []
    for name in _lib.EXPORTS:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    gc.collect()
    m = NoiseModel()
    m.load_state_dict(make_state_dict(0, False))
    m = m.cuda().train()
    fp = ForwardProcess()
    g = torch.Generator().manual_seed(0)
    x0 = (torch.rand(4, 1, 28, 28, generator=g) * 2 - 1).cuda()
    step = TrainStep(m, fp, lr=1e-3)
    step.step(x0)
    torch.cuda.synchronize()
    train_calls = list(calls)
    calls.clear()
    x = sample(m, ForwardProcess(num_timesteps=2), "cuda", n_samples=2)
    torch.cuda.synchronize()
    assert torch.isfinite(x).all()
    assert "tdx_unet_forward" in train_calls and any(c.startswith("tdx_unet_eval_step") or c == "tdx_unet_forward"
                                                     for c in calls)
    for name in NEW:
        assert name not in train_calls and name not in calls
    M.pair_gram(x0.reshape(4, 784), x0.reshape(4, 784))
    assert calls[-1] == "tdx_pair_gram"            # the recorder does see the new entries when they run
