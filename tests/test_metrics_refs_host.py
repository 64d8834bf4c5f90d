"""The references and bounds of tests/metrics_helpers.py against brute force, the host half of
tiny_diffusion_amd/metrics.py (the Frechet distance, the KID estimator and its subsets, argument validation) and the
binding of the five new entries.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import metrics_helpers as H

from tiny_diffusion_amd import _lib, metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tdx_pair_scratch_bytes", "tdx_pair_gram", "tdx_pair_kth_dist2", "tdx_pair_member", "tdx_pair_poly_rowsum")


# ------------------------------------------------------------------ helpers against brute force
def test_epilogue_references_match_brute_force():
    a, b = H.inputs(3, 7, 5, 3)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    g = np.array([[sum(a64[i, k] * b64[j, k] for k in range(3)) for j in range(5)] for i in range(7)])
    assert np.allclose(H.gram_ref(a, b), g, rtol=1e-14, atol=0)
    d2 = np.array([[sum((a64[i, k] - b64[j, k]) ** 2 for k in range(3)) for j in range(5)] for i in range(7)])
    assert np.allclose(H.dist2_ref(a, b), d2, rtol=1e-14, atol=0)
    for k in (1, 3, 5):
        assert np.array_equal(H.kth_dist2_ref(a, b, k), np.array([sorted(row)[k - 1] for row in H.dist2_ref(a, b)]))
    self_k2 = [sorted(v for j, v in enumerate(row) if j != i)[1] for i, row in enumerate(H.dist2_ref(a, a))]
    assert np.array_equal(H.kth_dist2_ref(a, a, 2, True), np.array(self_k2))
    r2 = np.array([0.5, 2.0, 0.1, 4.0, 1.0])
    flags = [int(any(d2[i, j] <= r2[j] for j in range(5))) for i in range(7)]
    assert H.member_ref(a, b, r2).tolist() == flags and 0 < sum(flags) < 7
    poly = [sum((0.25 * g[i, j] + 1.0) ** 3 for j in range(5) if j != i) for i in range(7)]
    assert np.allclose(H.poly_rowsum_ref(a, b, 0.25, 1.0, True), poly, rtol=1e-13, atol=0)


def test_fp32_evaluation_lies_within_the_bounds():
    """The kernels' operation order, restated in numpy fp32, is inside every bound - so the bounds are not vacuous for
    the arithmetic they are meant for - and a Gram matrix with one product dropped is outside."""
    a, b = H.inputs(0, 31, 33, 33)
    g = np.zeros((31, 33), np.float32)
    for k in range(33):   # products are exact in fp64; one rounding per step, like fmaf
        g = (g.astype(np.float64) + a[:, k:k + 1].astype(np.float64) * b[:, k].astype(np.float64)[None, :]).astype(np.float32)
    assert (np.abs(g - H.gram_ref(a, b)) <= H.gram_bound(a, b)).all()
    na = np.zeros(31, np.float32)
    nb = np.zeros(33, np.float32)
    for k in range(33):
        na = (na.astype(np.float64) + a[:, k].astype(np.float64) ** 2).astype(np.float32)
        nb = (nb.astype(np.float64) + b[:, k].astype(np.float64) ** 2).astype(np.float32)
    d2 = np.maximum(np.float32(0), (na[:, None] + nb[None, :]) - np.float32(2) * g)
    assert d2.dtype == np.float32 and (np.abs(d2 - H.dist2_ref(a, b)) <= H.dist2_bound(a, b)).all()
    dropped = g - a[:, 5:6] * b[:, 5][None, :]
    assert (np.abs(dropped - H.gram_ref(a, b)) > H.gram_bound(a, b)).any()


def test_decidability_rule_on_a_constructed_case():
    a = np.array([[0.0], [1.0], [3.0]], np.float32)
    b = np.array([[0.0], [10.0]], np.float32)
    r2, rb = np.array([1.0, 4.0]), np.array([1e-6, 1e-6])
    sin, sout = H.member_decidable(a, b, r2, rb)
    assert sin.tolist() == [True, False, False]       # 0 is well inside; 1 sits on the rim: undecided
    assert sout.tolist() == [False, False, True]
    assert H.member_ref(a, b, r2).tolist() == [1, 1, 0]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("d", [20, 33, 784])
@pytest.mark.parametrize("shift", [0.0, 0.3])
def test_the_gpu_cases_are_decidable_and_mixed(seed, d, shift):
    """The inputs of tests/test_gpu_metrics.py: the reference alone leaves no query out, and precision and recall are
    neither all 0 nor all 1."""
    x, y = H.centre_ref(*H.inputs(seed, 133, 70, d, shift))
    p, r, out_p, out_r = H.precision_recall_ref(x, y, 3)
    assert out_p == 0 and out_r == 0
    assert 0.0 < p < 1.0 and 0.0 < r < 1.0, (p, r)   # the twelve cases span 0.04 .. 0.85


# ------------------------------------------------------------------ Frechet distance (host fp64)
def _random_moments(seed, d, n):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, d)) @ rng.standard_normal((d, d)) * 0.5 + rng.standard_normal(d)
    return f.mean(axis=0), np.cov(f, rowvar=False).reshape(d, d)


@pytest.mark.parametrize("d", [1, 20, 96])
def test_frechet_distance_against_the_product_eigenvalues(d):
    mu_a, cov_a = _random_moments(0, d, 4 * d + 8)
    mu_b, cov_b = _random_moments(1, d, 4 * d + 8)
    tol = 1e-8 * (np.trace(cov_a) + np.trace(cov_b))
    fd = M.frechet_from_moments(mu_a, cov_a, mu_b, cov_b)
    assert abs(fd - H.frechet_ref(mu_a, cov_a, mu_b, cov_b)) <= tol
    assert abs(M.frechet_from_moments(mu_a, cov_a, mu_a, cov_a)) <= tol
    assert fd > 0


def test_frechet_distance_of_diagonal_gaussians():
    rng = np.random.default_rng(5)
    d = 784
    mu_a, mu_b = rng.standard_normal(d), rng.standard_normal(d)
    sig_a, sig_b = rng.uniform(0.1, 2.0, d), rng.uniform(0.1, 2.0, d)
    fd = M.frechet_from_moments(mu_a, np.diag(sig_a ** 2), mu_b, np.diag(sig_b ** 2))
    tol = 1e-8 * ((sig_a ** 2).sum() + (sig_b ** 2).sum())
    assert abs(fd - H.frechet_diag(mu_a, sig_a, mu_b, sig_b)) <= tol


def test_frechet_distance_takes_stats_objects_and_checks_shapes():
    class S:
        def __init__(self, mu, cov):
            self._mu, self._cov = mu, cov

        def mean(self):
            return torch.from_numpy(self._mu)

        def cov(self):
            return torch.from_numpy(self._cov)

    mu_a, cov_a = _random_moments(2, 6, 40)
    mu_b, cov_b = _random_moments(3, 6, 40)
    assert M.frechet_distance(S(mu_a, cov_a), S(mu_b, cov_b)) == M.frechet_from_moments(mu_a, cov_a, mu_b, cov_b)
    with pytest.raises(ValueError):
        M.frechet_from_moments(mu_a, cov_a, mu_b[:5], cov_b)
    with pytest.raises(ValueError):
        M.FeatureStats().mean()


def test_frechet_bound_covers_a_perturbation_within_it():
    mu_a, cov_a = _random_moments(6, 12, 9)      # rank deficient: 9 samples in 12 dimensions
    mu_b, cov_b = _random_moments(7, 12, 60)
    rng = np.random.default_rng(8)
    eb = 1e-6 * np.abs(cov_a).max() * np.ones((12, 12))
    pert = rng.uniform(-1, 1, (12, 12)) * eb
    pert = np.triu(pert) + np.triu(pert, 1).T
    zero = np.zeros(12)
    bound = H.frechet_bound(mu_a, cov_a, mu_b, cov_b, zero, eb, zero, eb)
    moved = M.frechet_from_moments(mu_a, cov_a + pert, mu_b, cov_b - pert)
    assert abs(moved - M.frechet_from_moments(mu_a, cov_a, mu_b, cov_b)) <= bound


# ------------------------------------------------------------------ KID
def test_kid_estimator_matches_brute_force_and_its_closed_form_on_identical_sets():
    a, b = H.inputs(4, 9, 6, 5, 0.3)
    val, bound = H.kid_ref(a, b)
    assert abs(val - H.kid_brute(a, b)) <= 1e-12 * max(1.0, abs(val)) and bound > 0
    # identical sets: the cross sum is the within sum plus the diagonal, so
    # MMD^2 = 2 [ S / (m (m-1)) - (S + D) / m^2 ] with S the off-diagonal and D the diagonal kernel sum
    g = float(np.float32(1.0 / 5))
    kmat = (g * H.gram_ref(a, a) + 1.0) ** 3
    m = len(a)
    diag = np.trace(kmat)
    off = kmat.sum() - diag
    closed = 2.0 * (off / (m * (m - 1)) - (off + diag) / m ** 2)
    assert abs(H.kid_ref(a, a)[0] - closed) <= 1e-12 * abs(closed)
    assert abs(M.mmd2_from_rowsums(off, off, off + diag, m, m) - closed) <= 1e-12 * abs(closed)
    with pytest.raises(ValueError):
        M.mmd2_from_rowsums(0.0, 0.0, 0.0, 1, 5)


def test_kid_subsets_are_reproducible_under_the_seed():
    s0, s1, s2 = M.kid_subsets(50, 40, 16, 5, 7), M.kid_subsets(50, 40, 16, 5, 7), M.kid_subsets(50, 40, 16, 5, 8)
    assert len(s0) == 5
    for (ia, ib), (ja, jb) in zip(s0, s1):
        assert np.array_equal(ia, ja) and np.array_equal(ib, jb)
        assert len(set(ia.tolist())) == 16 and len(set(ib.tolist())) == 16 and ia.max() < 50 and ib.max() < 40
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(s0, s2))
    assert len(M.kid_subsets(50, 10, 16, 2, 0)[0][0]) == 10      # clipped to the smaller set
    for bad in ((50, 40, 1, 5, 0), (50, 40, 16, 0, 0), (50, 40, 16, 5, -1), (50, 1, 16, 5, 0)):
        with pytest.raises(ValueError):
            M.kid_subsets(*bad)


# ------------------------------------------------------------------ argument validation, before any launch
def test_bad_arguments_raise_before_any_launch(monkeypatch):
    launched = []
    for name in NEW[1:]:
        monkeypatch.setattr(_lib.lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    x = torch.zeros(6, 4)
    for k in (0, 9, True, 2.0):
        with pytest.raises(ValueError):
            M.pair_kth_dist2(x, x, k)
        with pytest.raises(ValueError):
            M.precision_recall(x, x, k=k)
    with pytest.raises(ValueError):
        M.pair_kth_dist2(x, x[:3], 3, exclude_diag=True)          # nb = k
    with pytest.raises(ValueError):
        M.precision_recall(x, x[:3], k=3)
    with pytest.raises(ValueError):
        M.pair_kth_dist2(x, x, 3, col_chunks=-1)
    for fn in (lambda t: M.pair_gram(t, t), lambda t: M.pair_kth_dist2(t, t, 3, True),
               lambda t: M.pair_member(t, t, torch.zeros(6)), lambda t: M.pair_poly_rowsum(t, t, 0.25, 1.0),
               lambda t: M.precision_recall(t, t), lambda t: M.kernel_distance(t, t), lambda t: M.features(t),
               lambda t: M.FeatureStats().update(t), lambda t: M.evaluate_samples(t, t)):
        with pytest.raises(_lib.TdxError):
            fn(x)                                                  # fp32 on the CPU: no fallback
        with pytest.raises(ValueError):
            fn(x.double())
    with pytest.raises(ValueError):
        M.pair_gram(x, torch.zeros(6, 5))
    with pytest.raises(ValueError):
        M.pair_gram(x[0], x)
    with pytest.raises(ValueError):
        M.features(x, extractor=3)
    assert launched == []


def test_scratch_size_refuses_what_the_entries_refuse():
    f = _lib.lib.tdx_pair_scratch_bytes
    assert f(0, 5, 1, 0) == 0 and f(5, 0, 1, 0) == 0 and f(5, 5, 9, 0) == 0 and f(5, 5, 1, -1) == 0
    # the norms (16-byte rounded) and one partial row of max(4 k, 8) bytes per query and chunk; chunks clipped to tiles
    assert f(133, 70, 3, 0) == 816 + 133 * 12
    assert f(300, 300, 8, 2) == 2400 + 2 * 300 * 32 and f(300, 300, 8, 5) == 2400 + 3 * 300 * 32
    assert f(300, 300, 0, 1) == 2400 + 300 * 8


# ------------------------------------------------------------------ symbols
def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "tdx.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
        assert re.search(r"\b%s\(" % name, header), name
    assert _lib.lib.tdx_version() == 400
