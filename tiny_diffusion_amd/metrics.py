"""Sample-quality metrics on any feature space: the Frechet distance (Heusel et al. 2017), the kernel distance KID
(Binkowski et al. 2018) and precision / recall (Kynkaanniemi et al. 2019, as guided-diffusion's evaluator computes
them).  No pretrained network is involved: ``features`` flattens raw pixels or latents, or runs an extractor - the
package's own ``VAE`` (the mean of ``encode``, 20-d) or any callable.

Everything that touches all pairs runs in the tiled fp32-MFMA kernels of csrc/metrics.hip (include/tdx.h,
``tdx_pair_*``): the pair matrix is reduced in the epilogue and never stored, except by ``tdx_pair_gram``, which the
covariance uses.  With X the real and Y the generated features:

    FD        = |mu_x - mu_y|^2 + tr S_x + tr S_y - 2 tr (S_x S_y)^(1/2)       fp64 on the host from FeatureStats
    KID       = sum_{i!=j} k(x_i,x_j) / (m (m-1)) + sum_{i!=j} k(y_i,y_j) / (n (n-1)) - 2 sum_ij k(x_i,y_j) / (m n),
                k(x, y) = (x.y / d + 1)^3                                       three tdx_pair_poly_rowsum calls
    r_x(i)^2  = k-th smallest |x_i - x_j|^2 over j != i                         tdx_pair_kth_dist2(X, X, exclude_diag)
    precision = mean_j [ some i: |y_j - x_i|^2 <= r_x(i)^2 ]                    tdx_pair_member(Y, X, r_x^2)
    recall    = mean_i [ some j: |x_i - y_j|^2 <= r_y(j)^2 ]                    tdx_pair_member(X, Y, r_y^2)

Inputs are fp32 CUDA tensors; there is no CPU fallback (``TdxError`` for a CPU tensor, ``ValueError`` for another dtype
or shape, both before any launch).  Not here: density / coverage, a learned or pretrained feature network, gathering
features across GPUs."""
from __future__ import annotations

import numbers
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib

__all__ = ["features", "FeatureStats", "frechet_distance", "frechet_from_moments", "kernel_distance", "kid_subsets",
           "mmd2_from_rowsums", "centre_on", "precision_recall", "evaluate_samples", "pair_gram", "pair_kth_dist2", "pair_member",
           "pair_poly_rowsum", "KernelDistance", "PrecisionRecall", "SampleQuality", "K_MAX", "GRAM_ROWS"]

KernelDistance = namedtuple("KernelDistance", ["kid", "std"])
PrecisionRecall = namedtuple("PrecisionRecall", ["precision", "recall"])
SampleQuality = namedtuple("SampleQuality", ["fd", "kid", "precision", "recall"])

K_MAX = 8          # the longest k-smallest list tdx_pair_kth_dist2 keeps
GRAM_ROWS = 4096   # FeatureStats: rows of a batch per tdx_pair_gram call


def _int(v, name, lo):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral) or v < lo:
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return int(v)


def _shape_dtype(f, name):
    if not isinstance(f, torch.Tensor) or f.dim() != 2 or f.shape[0] < 1 or f.shape[1] < 1:
        raise ValueError(f"{name} must be a tensor (N, d) with N, d >= 1")
    if f.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {f.dtype}")


def _on_gpu(f):
    if not f.is_cuda:
        raise _lib.TdxError("the sample-quality metrics run on the GPU only (no CPU fallback)")
    return f.detach().contiguous()


def _matrix(f, name):
    """The checked (N, d) fp32 CUDA matrix, contiguous."""
    _shape_dtype(f, name)
    return _on_gpu(f)


def _pair(a, b):
    _shape_dtype(a, "a")
    _shape_dtype(b, "b")
    if a.shape[1] != b.shape[1] or a.device != b.device:
        raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} must share d and the device")
    return _on_gpu(a), _on_gpu(b)


def _k(k, nb, exclude_diag):
    k = _int(k, "k", 1)
    if k > K_MAX:
        raise ValueError(f"k must be <= {K_MAX}, got {k}")
    if nb < k + (1 if exclude_diag else 0):
        raise ValueError(f"k = {k} needs at least {k + (1 if exclude_diag else 0)} candidates, got {nb}")
    return k


def _scratch(na, nb, k, col_chunks, device):
    n = lib.tdx_pair_scratch_bytes(na, nb, k, col_chunks)
    if n == 0:
        raise ValueError(f"no scratch size for na={na}, nb={nb}, k={k}, col_chunks={col_chunks}")
    return torch.empty((n + 7) // 8, dtype=torch.float64, device=device), n


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def pair_gram(a, b):
    """``a @ b.T`` (na, nb) in fp32 by ``tdx_pair_gram``: every element the k-ordered fmaf chain of the fp32 MFMA."""
    a, b = _pair(a, b)
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
    check(lib.tdx_pair_gram(a.data_ptr(), b.data_ptr(), a.shape[0], b.shape[0], a.shape[1], out.data_ptr(), _stream(a)),
          "tdx_pair_gram")
    return out


def pair_kth_dist2(a, b, k, exclude_diag=False, col_chunks=0):
    """(na,) fp32: the k-th smallest squared distance from every row of ``a`` to the rows of ``b``
    (``exclude_diag``: without row i of ``b``, by index)."""
    col_chunks = _int(col_chunks, "col_chunks", 0)
    if isinstance(b, torch.Tensor) and b.dim() == 2:
        k = _k(k, b.shape[0], exclude_diag)
    a, b = _pair(a, b)
    na, nb, d = a.shape[0], b.shape[0], a.shape[1]
    out = torch.empty(na, dtype=torch.float32, device=a.device)
    ws, n = _scratch(na, nb, k, col_chunks, a.device)
    check(lib.tdx_pair_kth_dist2(a.data_ptr(), b.data_ptr(), na, nb, d, k, int(bool(exclude_diag)), col_chunks,
                                 out.data_ptr(), ws.data_ptr(), n, _stream(a)), "tdx_pair_kth_dist2")
    return out


def pair_member(a, b, r2, col_chunks=0):
    """(na,) int32: 1 where the row of ``a`` lies within ``sqrt(r2[j])`` of some row j of ``b``."""
    col_chunks = _int(col_chunks, "col_chunks", 0)
    a, b = _pair(a, b)
    na, nb, d = a.shape[0], b.shape[0], a.shape[1]
    if not isinstance(r2, torch.Tensor) or r2.dtype != torch.float32 or tuple(r2.shape) != (nb,) or r2.device != b.device:
        raise ValueError(f"r2 must be a float32 tensor ({nb},) on the device of b: one squared radius per candidate")
    r2 = r2.detach().contiguous()
    out = torch.empty(na, dtype=torch.int32, device=a.device)
    ws, n = _scratch(na, nb, 0, col_chunks, a.device)
    check(lib.tdx_pair_member(a.data_ptr(), b.data_ptr(), r2.data_ptr(), na, nb, d, col_chunks, out.data_ptr(),
                              ws.data_ptr(), n, _stream(a)), "tdx_pair_member")
    return out


def pair_poly_rowsum(a, b, gamma, coef0, exclude_diag=False, col_chunks=0):
    """(na,) fp64: ``sum_j (gamma a_i.b_j + coef0)^3`` (``exclude_diag``: j != i)."""
    col_chunks = _int(col_chunks, "col_chunks", 0)
    a, b = _pair(a, b)
    na, nb, d = a.shape[0], b.shape[0], a.shape[1]
    out = torch.empty(na, dtype=torch.float64, device=a.device)
    ws, n = _scratch(na, nb, 0, col_chunks, a.device)
    check(lib.tdx_pair_poly_rowsum(a.data_ptr(), b.data_ptr(), na, nb, d, float(gamma), float(coef0),
                                   int(bool(exclude_diag)), col_chunks, out.data_ptr(), ws.data_ptr(), n, _stream(a)),
          "tdx_pair_poly_rowsum")
    return out


@torch.no_grad()
def features(x, extractor=None):
    """``x`` (N, ...) as an (N, d) fp32 matrix on its device.  ``extractor=None``: the flattened values (raw pixels or
    latents); a ``VAE``: the mean of ``encode`` on the flattened input; any other callable: its output, flattened."""
    if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[0] < 1:
        raise ValueError("x must be a tensor (N, ...) with N >= 1")
    if x.dtype != torch.float32:
        raise ValueError(f"x must be float32, got {x.dtype}")
    if extractor is not None and not callable(extractor):
        raise ValueError("extractor must be None, a VAE or a callable")
    if not x.is_cuda:
        raise _lib.TdxError("the sample-quality metrics run on the GPU only (no CPU fallback)")
    if extractor is None:
        f = x
    else:
        from .vae import VAE

        if isinstance(extractor, VAE):
            f = extractor.encode(x.reshape(x.shape[0], -1).contiguous())[0]
        else:
            f = extractor(x)
        if not isinstance(f, torch.Tensor) or f.dim() < 1 or f.shape[0] != x.shape[0]:
            raise ValueError("the extractor must return a tensor with one row per sample")
    return _matrix(f.reshape(f.shape[0], -1).float(), "the features")


class FeatureStats:
    """Streaming mean and covariance of a feature set.  ``update(f)`` adds a batch (N, d) and may be called while
    sampling.  Kept on the device in fp64: the count, the sum of X = fl32(f - pivot) and the second moment X^T X about
    the fixed ``pivot`` (the fp32 mean of the first batch), each batch's X^T X from ``tdx_pair_gram`` on the transposed
    X in row chunks of at most ``GRAM_ROWS``; torch adds the chunks.  ``mean()`` = pivot + sum / n and
    ``cov()`` = (X^T X - sum sum^T / n) / (n - 1) are fp64 on the host."""

    def __init__(self):
        self.count = 0
        self.pivot = None
        self._sum = None
        self._m2 = None

    @torch.no_grad()
    def update(self, f):
        f = _matrix(f, "f")
        if self.pivot is None:
            self.pivot = f.double().mean(dim=0).float()
            self._sum = torch.zeros(f.shape[1], dtype=torch.float64, device=f.device)
            self._m2 = torch.zeros(f.shape[1], f.shape[1], dtype=torch.float64, device=f.device)
        elif f.shape[1] != self.pivot.shape[0] or f.device != self.pivot.device:
            raise ValueError("every batch must have the feature width and the device of the first")
        for r0 in range(0, f.shape[0], GRAM_ROWS):
            x = f[r0:r0 + GRAM_ROWS] - self.pivot
            xt = x.t().contiguous()
            self._sum += x.double().sum(dim=0)
            self._m2 += pair_gram(xt, xt).double()
        self.count += int(f.shape[0])
        return self

    def mean(self):
        if self.count < 1:
            raise ValueError("no features yet")
        return self.pivot.double().cpu() + self._sum.cpu() / self.count

    def cov(self):
        if self.count < 2:
            raise ValueError("the covariance needs at least two samples")
        s = self._sum.cpu()
        return (self._m2.cpu() - torch.outer(s, s) / self.count) / (self.count - 1)


def _psd_sqrt(m):
    w, v = torch.linalg.eigh(m)
    return (v * w.clamp_min(0.0).sqrt()) @ v.T


def frechet_from_moments(mu_a, cov_a, mu_b, cov_b):
    """The Frechet distance of N(mu_a, cov_a) and N(mu_b, cov_b) in fp64 on the host:
    tr (S_a S_b)^(1/2) is the sum of the square roots of the eigenvalues of S_a^(1/2) S_b S_a^(1/2), a symmetric
    positive semi-definite matrix (``torch.linalg.eigh`` on the CPU; negative roundings are clamped to 0)."""
    mu_a, mu_b = (torch.as_tensor(m, dtype=torch.float64, device="cpu") for m in (mu_a, mu_b))
    cov_a, cov_b = (torch.as_tensor(c, dtype=torch.float64, device="cpu") for c in (cov_a, cov_b))
    d = mu_a.shape[0]
    if mu_a.dim() != 1 or mu_b.shape != (d,) or cov_a.shape != (d, d) or cov_b.shape != (d, d):
        raise ValueError("means (d,) and covariances (d, d) of one width are needed")
    cov_a, cov_b = (cov_a + cov_a.T) / 2, (cov_b + cov_b.T) / 2
    ra = _psd_sqrt(cov_a)
    m = ra @ cov_b @ ra
    lam = torch.linalg.eigvalsh((m + m.T) / 2).clamp_min(0.0)
    diff = mu_a - mu_b
    return float(diff @ diff + torch.trace(cov_a) + torch.trace(cov_b) - 2.0 * lam.sqrt().sum())


def frechet_distance(stats_a, stats_b):
    """``frechet_from_moments`` of two ``FeatureStats`` (or anything with ``mean()`` and ``cov()``)."""
    return frechet_from_moments(stats_a.mean(), stats_a.cov(), stats_b.mean(), stats_b.cov())


def mmd2_from_rowsums(s_aa, s_bb, s_ab, m, n):
    """The unbiased MMD^2 from the three sums of kernel values: ``s_aa`` over i != j of the first set (m rows),
    ``s_bb`` likewise of the second (n rows), ``s_ab`` over all m n cross pairs."""
    if m < 2 or n < 2:
        raise ValueError("the unbiased estimator needs at least two samples per set")
    return s_aa / (m * (m - 1)) + s_bb / (n * (n - 1)) - 2.0 * s_ab / (m * n)


def kid_subsets(na, nb, subset_size, n_subsets, seed):
    """The row indices of the ``n_subsets`` seeded subsets: a list of ``(idx_a, idx_b)`` int64 arrays of
    ``min(subset_size, na, nb)`` distinct rows each, drawn by ``np.random.default_rng(seed)`` in this order."""
    subset_size, n_subsets = _int(subset_size, "subset_size", 2), _int(n_subsets, "n_subsets", 1)
    seed = _int(seed, "seed", 0)
    m = min(subset_size, na, nb)
    if m < 2:
        raise ValueError("a subset needs at least two samples per set")
    rng = np.random.default_rng(seed)
    return [(rng.choice(na, m, replace=False).astype(np.int64), rng.choice(nb, m, replace=False).astype(np.int64))
            for _ in range(n_subsets)]


def _mmd2(fa, fb):
    d = fa.shape[1]
    gamma = 1.0 / d
    s_aa = pair_poly_rowsum(fa, fa, gamma, 1.0, exclude_diag=True).sum()
    s_bb = pair_poly_rowsum(fb, fb, gamma, 1.0, exclude_diag=True).sum()
    s_ab = pair_poly_rowsum(fa, fb, gamma, 1.0).sum()
    return mmd2_from_rowsums(s_aa, s_bb, s_ab, fa.shape[0], fb.shape[0])


@torch.no_grad()
def kernel_distance(fa, fb, subset_size=None, n_subsets=100, seed=0):
    """KID: the unbiased MMD^2 under k(x, y) = (x.y / d + 1)^3, ``gamma = fl32(1 / d)``.  ``subset_size=None``: one
    estimate over the full sets, ``std`` 0; otherwise the mean and the (population) standard deviation over
    ``kid_subsets``.  Returns ``KernelDistance(kid, std)``, Python floats."""
    if subset_size is not None:
        subset_size, n_subsets = _int(subset_size, "subset_size", 2), _int(n_subsets, "n_subsets", 1)
        _int(seed, "seed", 0)
    fa, fb = _pair(fa, fb)
    if fa.shape[0] < 2 or fb.shape[0] < 2:
        raise ValueError("the unbiased estimator needs at least two samples per set")
    if subset_size is None:
        return KernelDistance(float(_mmd2(fa, fb)), 0.0)
    vals = []
    for ia, ib in kid_subsets(fa.shape[0], fb.shape[0], subset_size, n_subsets, seed):
        vals.append(_mmd2(fa[torch.from_numpy(ia).to(fa.device)], fb[torch.from_numpy(ib).to(fb.device)]))
    vals = torch.stack(vals).cpu()
    return KernelDistance(float(vals.mean()), float(vals.std(unbiased=False)))


def centre_on(f_real, f_gen):
    """Both sets minus the fp32 mean of the real set: distances are translation invariant, and smaller norms shrink the
    fp32 cancellation in |a|^2 + |b|^2 - 2 a.b."""
    c = f_real.double().mean(dim=0).float()
    return (f_real - c).contiguous(), (f_gen - c).contiguous()


@torch.no_grad()
def precision_recall(f_real, f_gen, k=3):
    """``PrecisionRecall(precision, recall)``: the fraction of generated samples inside the k-th-neighbour ball of some
    real sample, and the fraction of real samples inside the ball of some generated one."""
    k = _int(k, "k", 1)
    for f in (f_real, f_gen):
        if isinstance(f, torch.Tensor) and f.dim() == 2:
            _k(k, f.shape[0], True)
    f_real, f_gen = _pair(f_real, f_gen)
    x, y = centre_on(f_real, f_gen)
    r2_x = pair_kth_dist2(x, x, k, exclude_diag=True)
    r2_y = pair_kth_dist2(y, y, k, exclude_diag=True)
    inside_real, inside_gen = pair_member(y, x, r2_x).sum(), pair_member(x, y, r2_y).sum()
    return PrecisionRecall(int(inside_real) / y.shape[0], int(inside_gen) / x.shape[0])   # counts: one rounding each


@torch.no_grad()
def evaluate_samples(real, generated, extractor=None, k=3):
    """``SampleQuality(fd, kid, precision, recall)`` of ``generated`` against ``real`` in the feature space of
    ``features(., extractor)``; KID over the full sets."""
    fr, fg = features(real, extractor), features(generated, extractor)
    fd = frechet_distance(FeatureStats().update(fr), FeatureStats().update(fg))
    pr = precision_recall(fr, fg, k)
    return SampleQuality(fd, kernel_distance(fr, fg).kid, pr.precision, pr.recall)
