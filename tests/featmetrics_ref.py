"""numpy fp64 restatement of the distribution metrics (csrc/featmetrics.hip, lib/fid/dist_metrics.py) and the rounding bounds the
GPU tests hold the device to. Written for this feature: the reference project has no KID and no precision / recall.

Bounds, u = 2^-53, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1):
  Gram element   gamma(d + 3) sum_k |a_k| |b_k|: a dot product of length d summed in ANY order errs by at most gamma(d) sum|a_k b_k|
                 (the MFMA's grouping by four is one such order; products of widened fp32 values are exact), doubled plus slack because
                 the value it is compared with carries the same kind of error.
  KID sum        k = t^3, t = G / d + 1. To first order |dk| <= 3 tbar^2 e_G / d with tbar = |G| / d + 1 + e_G / d, plus the rounding
                 of the division, the addition, the two multiplications and the `count` additions: gamma(count + 4) sum |k|.
  KID            (e_xx + e_yy) / (m (m - 1)) + 2 e_xy / m^2 per subset, averaged."""
import numpy as np

U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- definitions -----------------------------------------------------------------------------------------------------------------

def gram(A, ia, B, ib):
    """G[i][j] = A[ia[i]] . B[ib[j]] in fp64 (ia / ib None: every row in order)."""
    a = np.asarray(A, dtype=np.float64)
    b = np.asarray(B, dtype=np.float64)
    a = a if ia is None else a[np.asarray(ia)]
    b = b if ib is None else b[np.asarray(ib)]
    return a @ b.T


def poly_kernel(G, d):
    t = G / float(d) + 1.0
    return t * t * t


def kid_sums(X, Y, ix, iy):
    """(num_subsets, 3): sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i,j} k(x_i, y_j); the diagonal left out by position."""
    ix, iy = np.asarray(ix), np.asarray(iy)
    d = X.shape[1]
    out = np.zeros((ix.shape[0], 3))
    for s in range(ix.shape[0]):
        off = ~np.eye(ix.shape[1], dtype=bool)
        out[s, 0] = poly_kernel(gram(X, ix[s], X, ix[s]), d)[off].sum()
        out[s, 1] = poly_kernel(gram(Y, iy[s], Y, iy[s]), d)[off].sum()
        out[s, 2] = poly_kernel(gram(X, ix[s], Y, iy[s]), d).sum()
    return out


def draw_subsets(seed, n_real, n_fake, m, num_subsets):
    """The draw of kernel_inception_distance: np.random.RandomState(seed); per subset in turn m fake rows, then m real rows, each
    without replacement. Returns (real_idx, fake_idx), (num_subsets, m) each."""
    rs = np.random.RandomState(seed)
    ir, jf = [], []
    for _ in range(num_subsets):
        jf.append(rs.choice(n_fake, m, replace=False))
        ir.append(rs.choice(n_real, m, replace=False))
    return np.array(ir), np.array(jf)


def kid_indices(n_real, n_fake, num_subsets, max_subset_size, seed):
    """(m, real_idx, fake_idx) as kernel_inception_distance uses them: when m == n_real == n_fake one subset over all rows in order."""
    m = min(n_real, n_fake, max_subset_size)
    if m == n_real == n_fake:
        return m, np.arange(m)[None], np.arange(m)[None]
    ir, jf = draw_subsets(seed, n_real, n_fake, m, num_subsets)
    return m, ir, jf


def kid_from_sums(sums, m):
    sums = np.asarray(sums, dtype=np.float64)
    return float(np.mean(sums[:, 0] / (m * (m - 1)) + sums[:, 1] / (m * (m - 1)) - 2.0 * sums[:, 2] / (m * m)))


def kid(real, fake, num_subsets=100, max_subset_size=1000, seed=0):
    m, ir, jf = kid_indices(real.shape[0], fake.shape[0], num_subsets, max_subset_size, seed)
    return kid_from_sums(kid_sums(real, fake, ir, jf), m)


def sq_dists(A, B):
    """D_ij = max(0, |a_i|^2 + |b_j|^2 - 2 a_i . b_j) in fp64."""
    a = np.asarray(A, dtype=np.float64)
    b = np.asarray(B, dtype=np.float64)
    return np.maximum(0.0, ((a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :]) - 2.0 * (a @ b.T))


def knn_radii(A, k):
    """The k-th smallest D_ij over j != i per row (self excluded by index)."""
    D = sq_dists(A, A)
    np.fill_diagonal(D, np.inf)
    return np.sort(D, axis=1)[:, k - 1]


def members(A, radii, B):
    """member[j] = any_i D(a_i, b_j) <= radii[i]."""
    return (sq_dists(A, B) <= np.asarray(radii)[:, None]).any(axis=0)


def precision_recall(real, fake, k=3):
    if real.shape[0] <= k or fake.shape[0] <= k:
        raise ValueError("more than k rows needed")
    p = members(real, knn_radii(real, k), fake).mean()
    r = members(fake, knn_radii(fake, k), real).mean()
    return float(p), float(r)


def pr_margin(real, fake, k=3):
    """Smallest relative distance (in units of the largest D) of any decision of precision_recall from flipping: |D_ij - r_i| over
    every membership comparison, and the gap between every row's k-th and (k+1)-th neighbour. The GPU test may demand equal
    precision / recall only where this is far above fp64 rounding."""
    worst, scale = np.inf, 0.0
    for A, Bm in ((real, fake), (fake, real)):
        D = sq_dists(A, A)
        scale = max(scale, float(D.max()))
        np.fill_diagonal(D, np.inf)
        S = np.sort(D, axis=1)
        if S.shape[1] - 1 > k:     # a (k+1)-th neighbour exists
            worst = min(worst, float((S[:, k] - S[:, k - 1]).min()))
        Dab = sq_dists(A, Bm)
        scale = max(scale, float(Dab.max()))
        worst = min(worst, float(np.abs(Dab - S[:, k - 1][:, None]).min()))
    return worst / scale


# ---- bounds ----------------------------------------------------------------------------------------------------------------------

def gram_bound(A, ia, B, ib):
    a = np.abs(np.asarray(A, dtype=np.float64))
    b = np.abs(np.asarray(B, dtype=np.float64))
    return gamma(A.shape[1] + 3) * gram(a, ia, b, ib)


def _kid_sum_bound_one(A, ia, B, ib, skip_diag):
    d = A.shape[1]
    G, eG = gram(A, ia, B, ib), gram_bound(A, ia, B, ib)
    tbar = np.abs(G) / d + 1.0 + eG / d
    first = 3.0 * tbar * tbar * eG / d
    absk = np.abs(poly_kernel(G, d))
    if skip_diag:
        off = ~np.eye(G.shape[0], dtype=bool)
        first, absk = first[off], absk[off]
    return float(first.sum() + gamma(first.size + 4) * absk.sum())


def kid_sum_bounds(X, Y, ix, iy):
    """(num_subsets, 3) bounds for kid_sums."""
    ix, iy = np.asarray(ix), np.asarray(iy)
    return np.array([[_kid_sum_bound_one(X, ix[s], X, ix[s], True), _kid_sum_bound_one(Y, iy[s], Y, iy[s], True),
                      _kid_sum_bound_one(X, ix[s], Y, iy[s], False)] for s in range(ix.shape[0])])


def kid_bound(sum_bounds, m):
    e = np.asarray(sum_bounds, dtype=np.float64)
    return float(np.mean((e[:, 0] + e[:, 1]) / (m * (m - 1)) + 2.0 * e[:, 2] / (m * m)))


def radius_bound(A, k):
    """4 gamma(d + 3) (|a_i|^2 + |a_j|^2), j the row's k-th neighbour here: |a_i|^2, |a_j|^2 and 2 G_ij each err by at most gamma(d)
    times a quantity <= |a_i|^2 + |a_j|^2 (Cauchy-Schwarz for the product term). Both sides name the same neighbour wherever the
    gap to the next one is above rounding (pr_margin); among exact ties the radius is the same whichever row is named."""
    n2 = (np.asarray(A, dtype=np.float64) ** 2).sum(axis=1)
    D = sq_dists(A, A)
    np.fill_diagonal(D, np.inf)
    j = np.argsort(D, axis=1, kind="stable")[:, k - 1]
    return 4.0 * gamma(A.shape[1] + 3) * (n2 + n2[j])
