"""CPU tier: the numpy restatement of KID and precision / recall (tests/featmetrics_ref.py) against independent formulations, its
rounding bounds against a longdouble evaluation, the conditions that let the GPU tier demand equal precision / recall, and the
command line's refusal of --dist-metrics without --fid-weights."""
import numpy as np
import pytest
import torch

import featmetrics_ref as F

PR_CASES = ((37, 29, 257, 7), (130, 33, 64, 10), (5, 5, 3, 9))     # (n_real, n_fake, d, seed), k = 3


def pr_inputs(n_r, n_f, d, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    real = rng.random((n_r, d)).astype(np.float32)
    fake = (1.05 * rng.random((n_f, d))).astype(np.float32)
    return real, fake


def _feats(seed, n, d):
    return np.random.Generator(np.random.PCG64(seed)).random((n, d)).astype(np.float32)


@pytest.mark.parametrize("n,d,k", [(23, 17, 1), (40, 64, 3), (9, 5, 5)])
def test_radii_and_membership_match_cdist_topk(n, d, k):
    a, b = _feats(1, n, d), _feats(2, n + 3, d) * 1.1
    ta, tb = torch.from_numpy(a).double(), torch.from_numpy(b).double()
    D = torch.cdist(ta, ta, p=2) ** 2
    D[torch.arange(n), torch.arange(n)] = float("inf")
    want = torch.topk(D, k, dim=1, largest=False).values[:, k - 1].numpy()
    got = F.knn_radii(a, k)
    assert np.abs(got - want).max() <= 1e-12 * want.max()
    Dab = (torch.cdist(ta, tb, p=2) ** 2).numpy()
    margin = np.abs(Dab - want[:, None]).min()
    assert margin > 1e-9 * Dab.max()                      # no decision near a tie: the two formulations must agree exactly
    assert np.array_equal(F.members(a, got, b), (Dab <= want[:, None]).any(axis=0))
    p, r = F.precision_recall(a, b, k)
    assert 0.0 <= p <= 1.0 and 0.0 <= r <= 1.0


def _kid_sums_longdouble(X, Y, ix, iy):
    L = np.longdouble
    d = X.shape[1]
    out = np.zeros((len(ix), 3), dtype=L)
    for s in range(len(ix)):
        for q, (P, ip, Q, iq, skip) in enumerate(((X, ix[s], X, ix[s], True), (Y, iy[s], Y, iy[s], True), (X, ix[s], Y, iy[s], False))):
            acc = L(0)
            for i in range(len(ip)):
                for j in range(len(iq)):
                    if skip and i == j:
                        continue
                    g = L(0)
                    for kk in range(d):
                        g += L(P[ip[i], kk]) * L(Q[iq[j], kk])
                    t = g / L(d) + L(1)
                    acc += t * t * t
            out[s, q] = acc
    return out


@pytest.mark.parametrize("m,d", [(2, 3), (5, 17), (7, 4)])
def test_kid_sums_match_an_explicit_longdouble_loop(m, d):
    X, Y = _feats(3, 11, d), _feats(4, 9, d) * 1.2
    rs = np.random.RandomState(0)
    ix = np.array([rs.choice(11, m, replace=False) for _ in range(2)])
    iy = np.array([rs.choice(9, m, replace=False) for _ in range(2)])
    ix[1, 1] = ix[1, 0]                                   # a row drawn twice: only the position pair (i, i) is left out
    want = _kid_sums_longdouble(X, Y, ix, iy)
    got = F.kid_sums(X, Y, ix, iy)
    bound = F.kid_sum_bounds(X, Y, ix, iy)
    assert (np.abs(got - want) <= bound).all()
    assert (bound < 1e-12 * np.abs(got)).all()            # and the bound is a rounding bound, not a loose one
    assert F.kid_from_sums(got, m) == pytest.approx(float((want[:, 0] + want[:, 1]).mean() / (m * (m - 1)) - 2 * want[:, 2].mean() / m ** 2),
                                                    abs=F.kid_bound(bound, m) + 1e-18)


def test_bounds_hold_for_shuffled_fp64_summation():
    L = np.longdouble
    rng = np.random.Generator(np.random.PCG64(11))
    d, m = 257, 6
    X, Y = _feats(5, m, d), _feats(6, m, d) - 0.3
    exact = (X.astype(L)[:, None, :] * Y.astype(L)[None, :, :]).sum(axis=2)
    gb = F.gram_bound(X, None, Y, None)
    for _ in range(5):
        perm = rng.permutation(d)
        G = np.zeros((m, m))
        for i in range(m):
            for j in range(m):
                acc = 0.0
                for kk in perm:                            # one fp64 rounding per addition, in shuffled order
                    acc += float(X[i, kk]) * float(Y[j, kk])
                G[i, j] = acc
        assert (np.abs(G.astype(L) - exact) <= gb).all()
        # the KID sum from that Gram matrix, its terms added in shuffled order
        k = F.poly_kernel(G, d).ravel()
        acc = 0.0
        for v in k[rng.permutation(k.size)]:
            acc += v
        t = exact / L(d) + L(1)
        want = (t * t * t).sum()
        bound = F.kid_sum_bounds(X, Y, np.arange(m)[None], np.arange(m)[None])[0, 2]
        assert abs(L(acc) - want) <= bound


def test_index_draw_is_a_pure_function_of_seed_and_sizes():
    a = F.draw_subsets(3, 70, 67, 32, 5)
    b = F.draw_subsets(3, 70, 67, 32, 5)
    c = F.draw_subsets(4, 70, 67, 32, 5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0])
    assert a[0].shape == a[1].shape == (5, 32)
    for s in range(5):
        assert len(set(a[0][s])) == 32 and len(set(a[1][s])) == 32 and a[0][s].max() < 70 and a[1][s].max() < 67
    # fake first, then real, per subset in turn
    rs = np.random.RandomState(3)
    assert np.array_equal(rs.choice(67, 32, replace=False), a[1][0]) and np.array_equal(rs.choice(70, 32, replace=False), a[0][0])
    m, ir, jf = F.kid_indices(20, 20, 100, 1000, 0)
    assert m == 20 and np.array_equal(ir, np.arange(20)[None]) and np.array_equal(jf, np.arange(20)[None])
    # the product draws the same lists
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.fid import dist_metrics
    p = dist_metrics.draw_subsets(3, 70, 67, 32, 5)
    assert np.array_equal(p[0], a[0]) and np.array_equal(p[1], a[1])


@pytest.mark.parametrize("case", PR_CASES)
def test_named_precision_recall_inputs_have_no_near_ties(case):
    real, fake = pr_inputs(*case)
    margin = F.pr_margin(real, fake, 3)
    print(f"precision/recall inputs {case}: smallest relative gap {margin:.3e}")
    assert margin > 1e-9
    p, r = F.precision_recall(real, fake, 3)
    print(f"precision {p:.3f} recall {r:.3f}")
    if case[0] > 5:
        assert 0.0 < p < 1.0 and 0.0 < r < 1.0            # a constant answer cannot pass the GPU comparison


def test_dist_metrics_without_fid_weights_is_refused_before_any_device_work(capsys):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import train
    with pytest.raises(SystemExit):
        train.main(["-exp", "minimaxgan_l1", "--dist-metrics", "kid"])
    assert "--dist-metrics needs --fid-weights" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.main(["-exp", "minimaxgan_l1", "--dist-metrics", "kid,fid", "--fid-weights", "x.pth"])
