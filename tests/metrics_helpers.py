"""fp64 numpy restatements of the pairwise kernels (include/tdx.h, tdx_pair_*) and of the metrics built on them
(tiny_diffusion_amd/metrics.py), with the error bounds the GPU tests hold the kernels to.  No GPU needed.

The bounds are the textbook ones for an fp32 dot product accumulated in order (Higham, Accuracy and Stability of
Numerical Algorithms, ch. 3), u = 2^-24 and gamma_n = n u / (1 - n u):

  Gram          |g - g_ref| <= gamma_d sum_k |a_k b_k|              d fused multiply-adds, one rounding each
  squared dist  |d2 - d2_ref| <= 2 (d + 8) u (|a|^2 + |b|^2)        the two norms (gamma_d each), the Gram term
                                                                    (2 gamma_d sum|a b| <= gamma_d (|a|^2 + |b|^2)),
                                                                    one add and one subtraction of values <= 2 (|a|^2 + |b|^2);
                                                                    the floor max(0, .) moves nothing further away
  k-th dist     an order statistic of a row moves by at most the largest perturbation in that row
  poly row sum  v = gamma g + c0 moves by e = |gamma| * Gram bound, so v^3 by (|v| + e)^3 - |v|^3; the fp64 arithmetic
                of the cube and of the nb-term sum adds at most (nb + 8) 2^-53 of the summed magnitudes
"""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


def inputs(seed, n_real, n_gen, d, shift=0.0):
    """The two fp32 sets of the tests: standard normal, the generated one shifted by ``shift`` per coordinate."""
    rng = np.random.default_rng(seed)
    real = rng.standard_normal((n_real, d)).astype(np.float32)
    gen = (rng.standard_normal((n_gen, d)) + shift).astype(np.float32)
    return real, gen


# ------------------------------------------------------------------ the four epilogues
def gram_ref(a, b):
    return a.astype(np.float64) @ b.astype(np.float64).T


def gram_bound(a, b):
    return gamma(a.shape[1]) * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64).T)


def _norms(x):
    x = x.astype(np.float64)
    return (x * x).sum(axis=1)


def dist2_ref(a, b):
    """(na, nb) exact squared distances, from the differences (no cancellation)."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    for i in range(a.shape[0]):
        diff = b - a[i]
        out[i] = (diff * diff).sum(axis=1)
    return out


def dist2_bound(a, b):
    d = a.shape[1]
    return 2.0 * (d + 8) * U * (_norms(a)[:, None] + _norms(b)[None, :])


def _mask_diag(m, exclude_diag, fill):
    if exclude_diag:
        m = m.copy()
        n = min(m.shape)
        m[np.arange(n), np.arange(n)] = fill
    return m


def kth_dist2_ref(a, b, k, exclude_diag=False):
    """The k-th smallest squared distance of every row of a, without candidate j == i (by index) when asked."""
    d2 = _mask_diag(dist2_ref(a, b), exclude_diag, np.inf)
    return np.sort(d2, axis=1)[:, k - 1]


def kth_dist2_bound(a, b, exclude_diag=False):
    return _mask_diag(dist2_bound(a, b), exclude_diag, 0.0).max(axis=1)


def member_ref(a, b, r2):
    """flag_i = any_j [ d2_ij <= r2_j ]: the radius is the candidate's."""
    return (dist2_ref(a, b) <= np.asarray(r2, dtype=np.float64)[None, :]).any(axis=1).astype(np.int32)


def member_decidable(a, b, r2_ref, r2_bound):
    """(surely_in, surely_out) boolean (na,): with tol_ij = the distance bound + the bound of candidate j's radius, a
    query is surely in when some pair has d2 - r2 < -tol and surely out when every pair has d2 - r2 > tol.  A query in
    neither is left out of the comparison."""
    margin = dist2_ref(a, b) - np.asarray(r2_ref, dtype=np.float64)[None, :]
    tol = dist2_bound(a, b) + np.asarray(r2_bound, dtype=np.float64)[None, :]
    return (margin < -tol).any(axis=1), (margin > tol).all(axis=1)


def poly_rowsum_ref(a, b, gamma32, coef0_32, exclude_diag=False):
    """sum_j (gamma g_ij + coef0)^3 in fp64 from the fp32 constants the kernel is given."""
    v = float(np.float32(gamma32)) * gram_ref(a, b) + float(np.float32(coef0_32))
    return _mask_diag(v ** 3, exclude_diag, 0.0).sum(axis=1)


def poly_rowsum_bound(a, b, gamma32, coef0_32, exclude_diag=False):
    g32 = abs(float(np.float32(gamma32)))
    v = np.abs(float(np.float32(gamma32)) * gram_ref(a, b) + float(np.float32(coef0_32)))
    hi = (v + g32 * gram_bound(a, b)) ** 3
    term = (hi - v ** 3) + 8 * U64 * hi
    term, hi = _mask_diag(term, exclude_diag, 0.0), _mask_diag(hi, exclude_diag, 0.0)
    return term.sum(axis=1) + b.shape[0] * U64 * hi.sum(axis=1)


# ------------------------------------------------------------------ the metrics
def centre_ref(real, gen):
    """What metrics.centre_on does: the fp64 mean of the real set rounded to fp32, subtracted in fp32."""
    c = real.astype(np.float64).mean(axis=0).astype(np.float32)
    return real - c, gen - c


def precision_recall_ref(x, y, k):
    """(precision, recall, left_out_precision, left_out_recall) from the centred sets x (real) and y (generated): the
    fp64 values, and how many queries of each direction the decidability rule leaves out."""
    r2_x, r2_y = kth_dist2_ref(x, x, k, True), kth_dist2_ref(y, y, k, True)
    bx, by = kth_dist2_bound(x, x, True), kth_dist2_bound(y, y, True)
    prec, rec = member_ref(y, x, r2_x), member_ref(x, y, r2_y)
    pin, pout = member_decidable(y, x, r2_x, bx)
    rin, rout = member_decidable(x, y, r2_y, by)
    return (int(prec.sum()) / prec.size, int(rec.sum()) / rec.size,   # a count over a count: one rounding
            int((~(pin | pout)).sum()), int((~(rin | rout)).sum()))


def mmd2(s_aa, s_bb, s_ab, m, n):
    return s_aa / (m * (m - 1)) + s_bb / (n * (n - 1)) - 2.0 * s_ab / (m * n)


def kid_ref(a, b):
    """The unbiased MMD^2 under (x.y / d + 1)^3 with gamma = fl32(1 / d), and the bound the row-sum bounds imply."""
    m, n, g = a.shape[0], b.shape[0], np.float32(1.0 / a.shape[1])
    s = [poly_rowsum_ref(a, a, g, 1.0, True), poly_rowsum_ref(b, b, g, 1.0, True), poly_rowsum_ref(a, b, g, 1.0)]
    e = [poly_rowsum_bound(a, a, g, 1.0, True), poly_rowsum_bound(b, b, g, 1.0, True), poly_rowsum_bound(a, b, g, 1.0)]
    # the three fp64 sums over the rows: m (or n) more roundings of the summed magnitudes
    e = [ei.sum() + len(si) * U64 * np.abs(si).sum() for si, ei in zip(s, e)]
    val = mmd2(s[0].sum(), s[1].sum(), s[2].sum(), m, n)
    return val, e[0] / (m * (m - 1)) + e[1] / (n * (n - 1)) + 2.0 * e[2] / (m * n)


def kid_brute(a, b):
    """The same estimator from explicit loops over the pairs (tiny cases)."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    g = float(np.float32(1.0 / a.shape[1]))
    k = lambda x, y: (g * float(x @ y) + 1.0) ** 3  # noqa: E731
    m, n = len(a), len(b)
    s_aa = sum(k(a[i], a[j]) for i in range(m) for j in range(m) if i != j)
    s_bb = sum(k(b[i], b[j]) for i in range(n) for j in range(n) if i != j)
    s_ab = sum(k(a[i], b[j]) for i in range(m) for j in range(n))
    return mmd2(s_aa, s_bb, s_ab, m, n)


def stats_ref(batches, pivot, chunk=4096):
    """FeatureStats restated: X = fl32(f - pivot) per batch, then fp64.  Returns (n, mean, cov, mean_bound, cov_bound):
    the covariance bound per element is the Gram bound of every chunk's X^T X (gamma of the chunk's rows) divided by
    n - 1, plus 2^-40 of the summed magnitudes for the fp64 sums (at most 2^13 roundings of 2^-53)."""
    pivot = np.asarray(pivot, dtype=np.float32)
    d = pivot.shape[0]
    n, s, sabs = 0, np.zeros(d), np.zeros(d)
    m2, bm2, am2 = np.zeros((d, d)), np.zeros((d, d)), np.zeros((d, d))
    for f in batches:
        for r0 in range(0, f.shape[0], chunk):
            x = (f[r0:r0 + chunk] - pivot).astype(np.float32)
            x64, xa = x.astype(np.float64), np.abs(x).astype(np.float64)
            s += x64.sum(axis=0)
            sabs += xa.sum(axis=0)
            m2 += x64.T @ x64
            am2 += xa.T @ xa
            bm2 += gamma(x.shape[0]) * (xa.T @ xa)
        n += f.shape[0]
    mean = pivot.astype(np.float64) + s / n
    cov = (m2 - np.outer(s, s) / n) / (n - 1)
    slack = 2.0 ** -40
    mean_bound = slack * (np.abs(pivot).astype(np.float64) + sabs / n)
    cov_bound = (bm2 + slack * (am2 + np.outer(sabs, sabs) / n)) / (n - 1)
    return n, mean, cov, mean_bound, cov_bound


def frechet_ref(mu_a, cov_a, mu_b, cov_b):
    """The Frechet distance by the formula independent of the library's: tr (S_a S_b)^(1/2) from the eigenvalues of
    the (non-symmetric) product S_a S_b - real parts, negative roundings clamped, square-rooted and summed."""
    lam = np.linalg.eigvals(cov_a @ cov_b).real
    diff = mu_a - mu_b
    return float(diff @ diff + np.trace(cov_a) + np.trace(cov_b) - 2.0 * np.sqrt(np.clip(lam, 0.0, None)).sum())


def frechet_diag(mu_a, sig_a, mu_b, sig_b):
    """Diagonal Gaussians in closed form: sum (sigma_a - sigma_b)^2 + |mu_a - mu_b|^2."""
    return float(((sig_a - sig_b) ** 2).sum() + ((mu_a - mu_b) ** 2).sum())


def frechet_bound(mu_a, cov_a, mu_b, cov_b, mean_bound_a, cov_bound_a, mean_bound_b, cov_bound_b):
    """How far the Frechet distance can move when every element of the means and covariances moves within its bound.

    The trace terms move by the summed diagonal bounds, the mean term by 2 |dmu| . e + |e|^2.  tr (S_a S_b)^(1/2) is
    the sum of the square roots of the eigenvalues lambda_i of S_b^(1/2) S_a S_b^(1/2).  Replacing S_a by S_a + E_a
    moves every sorted eigenvalue by at most |S_b|_2 |E_a|_F (Weyl), then S_b by S_b + E_b - the same spectrum seen as
    S_a'^(1/2) S_b S_a'^(1/2) - by at most (|S_a|_2 + |E_a|_F) |E_b|_F; fp64 eigenvalue solvers add d 2^-50 |S_a|_2 |S_b|_2
    on either side.  With delta their sum, |sqrt(l') - sqrt(l)| <= min(sqrt(delta), delta / sqrt(l)): the first holds
    for any l, l' >= 0 (this is what a rank-deficient covariance costs), the second because sqrt(l') + sqrt(l) >= sqrt(l)."""
    d = len(mu_a)
    ea_f, eb_f = np.linalg.norm(cov_bound_a), np.linalg.norm(cov_bound_b)
    na2, nb2 = np.linalg.norm(cov_a, 2), np.linalg.norm(cov_b, 2)
    delta = nb2 * ea_f + (na2 + ea_f) * eb_f + 2 * d * 2.0 ** -50 * (na2 + ea_f) * (nb2 + eb_f)
    lam = np.clip(np.linalg.eigvals(cov_a @ cov_b).real, 0.0, None)
    with np.errstate(divide="ignore"):
        per = np.minimum(np.sqrt(delta), delta / np.sqrt(lam))
    e_mu = mean_bound_a + mean_bound_b
    mean_term = 2.0 * (np.abs(mu_a - mu_b) * e_mu).sum() + (e_mu ** 2).sum()
    return float(mean_term + np.trace(cov_bound_a) + np.trace(cov_bound_b) + 2.0 * per.sum())
