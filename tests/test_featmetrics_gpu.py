"""GPU tier: the distribution-metric kernels (csrc/featmetrics.hip) and lib/fid/dist_metrics.py against the numpy fp64 restatement
tests/featmetrics_ref.py. Every bound is computed there from the test's own inputs (rounding analysis, no measured numbers);
where every product and sum is an exact integer or dyadic, and where no decision is near a tie (test_featmetrics_ref_cpu.py
checks that for the named inputs), the device must give the same bits / the same counts."""
import os
import pickle

import numpy as np
import pytest
import torch

import featmetrics_ref as F
from test_featmetrics_ref_cpu import PR_CASES, pr_inputs

pytestmark = pytest.mark.gpu


def _dm():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    from gan_inpainting_amd.lib.fid import dist_metrics
    return B, dist_metrics


def _rand(seed, n, d, signed=True):
    x = np.random.Generator(np.random.PCG64(seed)).random((n, d))
    return ((x - 0.5) * 3.0 if signed else x).astype(np.float32)


def _ints(seed, n, d, hi):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, hi + 1, (n, d)).astype(np.float32)


def _gram(A, ia, B_, ib):
    B, _ = _dm()
    a, b = torch.from_numpy(A).cuda(), torch.from_numpy(B_).cuda()
    na, nb = (A.shape[0] if ia is None else len(ia)), (B_.shape[0] if ib is None else len(ib))
    tia = None if ia is None else torch.from_numpy(np.asarray(ia, dtype=np.int32)).cuda()
    tib = None if ib is None else torch.from_numpy(np.asarray(ib, dtype=np.int32)).cuda()
    G = torch.full((na, nb), float("nan"), dtype=torch.float64, device="cuda")
    B.check(B.lib().gi_debug_feat_gram(B.get_ctx(a.device), B.ptr(a), B.ptr(tia), na, B.ptr(b), B.ptr(tib), nb, A.shape[1], B.ptr(G)))
    return G.cpu().numpy()


GRAM_CASES = [(1, 1, 1), (5, 7, 3), (17, 16, 4), (33, 65, 257), (64, 64, 2048), (130, 33, 1030)]


@pytest.mark.parametrize("na,nb,d", GRAM_CASES)
def test_gram_matches_the_restatement(na, nb, d):
    A, Bm = _rand(100 + na, na, d), _rand(200 + nb, nb, d)
    rng = np.random.Generator(np.random.PCG64(d))
    ia = rng.integers(0, na, na + 3)          # permutes and repeats rows
    ib = rng.integers(0, nb, nb + 2)
    for la, lb in ((None, None), (ia, ib)):
        got, ref, bound = _gram(A, la, Bm, lb), F.gram(A, la, Bm, lb), F.gram_bound(A, la, Bm, lb)
        err = np.abs(got - ref)
        print(f"gram ({na},{nb},{d}) lists={la is not None}: max err {err.max():.3e}, max err/bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert np.isfinite(got).all() and (err <= bound).all()
    Ai, Bi = _ints(1, na, d, 2), _ints(2, nb, d, 2)
    for la, lb in ((None, None), (ia, ib)):
        assert np.array_equal(_gram(Ai, la, Bi, lb), F.gram(Ai, la, Bi, lb))     # exact integers: the same bits


def test_gram_does_not_depend_on_position():
    A, Bm = _rand(7, 130, 257), _rand(8, 97, 257)
    rng = np.random.Generator(np.random.PCG64(3))
    pa, pb = rng.permutation(130), rng.permutation(97)
    G = _gram(A, None, Bm, None)
    assert np.array_equal(_gram(A, pa, Bm, pb), G[pa][:, pb])
    assert np.array_equal(_gram(A, pa[:5], Bm, pb[:70]), G[pa[:5]][:, pb[:70]])      # another call size, other tiles
    S = _gram(A, None, A, None)
    assert np.array_equal(S, S.T)                                                     # G_ij and G_ji: the same sum


def _kid_sums(X, Y, ix, iy):
    _, dm = _dm()
    return dm.kid_subset_sums(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), ix, iy).cpu().numpy()


def _lists(seed, n, m, subsets=3):
    rs = np.random.RandomState(seed)
    return np.array([rs.choice(n, m, replace=False) for _ in range(subsets)])


@pytest.mark.parametrize("d", [4, 257, 2048])
@pytest.mark.parametrize("m", [2, 17, 64, 130])
def test_kid_subset_sums_within_the_derived_bound(m, d):
    X, Y = _rand(11, 140, d), _rand(12, 133, d) * 1.1
    ix, iy = _lists(m, 140, m), _lists(m + 1, 133, m)
    got, ref, bound = _kid_sums(X, Y, ix, iy), F.kid_sums(X, Y, ix, iy), F.kid_sum_bounds(X, Y, ix, iy)
    err = np.abs(got - ref)
    print(f"kid sums m={m} d={d}: max err/bound {(err / bound).max():.3f}, max rel err {(err / np.abs(ref)).max():.3e}")
    assert got.shape == (3, 3) and (err <= bound).all()


@pytest.mark.parametrize("d", [4, 256, 2048])
@pytest.mark.parametrize("m", [2, 17, 64, 130])
def test_kid_subset_sums_exact_on_binary_features(m, d):
    X, Y = _ints(21, 140, d, 1), _ints(22, 133, d, 1)
    ix, iy = _lists(m, 140, m), _lists(m + 1, 133, m)
    assert np.array_equal(_kid_sums(X, Y, ix, iy), F.kid_sums(X, Y, ix, iy))      # dyadic G / d, 36-bit cubes, sums below 2^53


def test_kid_diagonal_is_skipped_by_index():
    X, Y = _ints(31, 40, 256, 1), _ints(32, 40, 256, 1)
    ix, iy = _lists(5, 40, 17), _lists(6, 40, 17)
    ix[0, 3] = ix[0, 9]            # one row twice in a subset: the pair (3, 9) is off the diagonal and counts, with k(x, x)
    iy[2, 0] = iy[2, 16]
    got, ref = _kid_sums(X, Y, ix, iy), F.kid_sums(X, Y, ix, iy)
    assert np.array_equal(got, ref)
    kxx = F.poly_kernel(F.gram(X, ix[0], X, ix[0]), 256)
    by_value = kxx.sum() - kxx[np.isclose(F.sq_dists(X[ix[0]], X[ix[0]]), 0.0)].sum()   # what skipping zero distances would give
    assert got[0, 0] != by_value


def test_kid_end_to_end():
    _, dm = _dm()
    real, fake = _rand(41, 70, 2048, signed=False), _rand(42, 67, 2048, signed=False) * 1.05
    tr, tf = torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda()
    got = dm.kernel_inception_distance(tr, tf, num_subsets=5, max_subset_size=32, seed=3)
    m, ir, jf = F.kid_indices(70, 67, 5, 32, 3)
    assert m == 32 and ir.shape == (5, 32)
    ref = F.kid(real, fake, 5, 32, 3)
    bound = F.kid_bound(F.kid_sum_bounds(real, fake, ir, jf), m)
    print(f"kid {got:.12e} ref {ref:.12e} err {abs(got - ref):.3e} bound {bound:.3e}")
    assert isinstance(got, float) and abs(got - ref) <= bound
    assert got != dm.kernel_inception_distance(tr, tf, num_subsets=5, max_subset_size=32, seed=4)
    # n_r = n_f = m: one subset over all rows, whatever num_subsets and seed say
    r20, f20 = real[:20], fake[:20]
    got1 = dm.kernel_inception_distance(tr[:20], tf[:20], num_subsets=7, seed=1)
    m1, i1, j1 = F.kid_indices(20, 20, 7, 1000, 1)
    assert i1.shape == (1, 20)
    assert abs(got1 - F.kid(r20, f20, 7, 1000, 1)) <= F.kid_bound(F.kid_sum_bounds(r20, f20, i1, j1), m1)
    assert got1 == dm.kernel_inception_distance(tr[:20], tf[:20], num_subsets=1, seed=9)
    with pytest.raises(ValueError):
        dm.kernel_inception_distance(tr[:1], tf)
    with pytest.raises(ValueError):
        dm.kid_subset_sums(tr, tf, np.array([[0, 70]]), np.array([[0, 1]]))       # an index outside its matrix: refused on the host


@pytest.mark.parametrize("case", PR_CASES)
def test_precision_recall_equals_the_restatement(case):
    _, dm = _dm()
    real, fake = pr_inputs(*case)
    tr, tf = torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda()
    assert dm.precision_recall(tr, tf, k=3) == F.precision_recall(real, fake, 3)
    for x, t in ((real, tr), (fake, tf)):
        got, ref, bound = dm.knn_radii(t, 3).cpu().numpy(), F.knn_radii(x, 3), F.radius_bound(x, 3)
        print(f"radii {case}: max err/bound {(np.abs(got - ref) / bound).max():.3f}")
        assert (np.abs(got - ref) <= bound).all()
    member, count = dm.manifold_members(tr, dm.knn_radii(tr, 3), tf)
    assert np.array_equal(member.cpu().numpy().astype(bool), F.members(real, F.knn_radii(real, 3), fake))
    assert int(count) == int(member.sum())


@pytest.mark.parametrize("k", [1, 3, 5])
def test_precision_recall_with_exact_ties(k):
    _, dm = _dm()
    real, fake = _ints(51, 40, 8, 1), _ints(52, 40, 8, 1)       # every distance a small integer: many equal ones, all exact
    tr, tf = torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda()
    assert np.array_equal(dm.knn_radii(tr, k).cpu().numpy(), F.knn_radii(real, k))
    assert dm.precision_recall(tr, tf, k=k) == F.precision_recall(real, fake, k)


def test_precision_recall_with_duplicated_rows_and_more_than_one_tile():
    _, dm = _dm()
    real, fake = _ints(61, 150, 16, 3), _ints(62, 70, 16, 3)
    real[100:110] = real[:10]                                    # copies are neighbours at distance 0, self is not
    fake[64] = fake[3]
    tr, tf = torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda()
    r1 = dm.knn_radii(tr, 1).cpu().numpy()
    assert np.array_equal(r1, F.knn_radii(real, 1)) and (r1[:10] == 0).all() and (r1[100:110] == 0).all()
    for k in (1, 2, 70):                                         # 70 > the 64 candidates a tile hands on
        assert np.array_equal(dm.knn_radii(tr, k).cpu().numpy(), F.knn_radii(real, k))
    assert dm.precision_recall(tr, tf, k=2) == F.precision_recall(real, fake, 2)


def test_precision_recall_refuses_too_few_rows():
    B, dm = _dm()
    x = torch.from_numpy(_rand(71, 5, 8)).cuda()
    with pytest.raises(ValueError):
        dm.precision_recall(x[:3], x, k=3)
    with pytest.raises(ValueError):
        dm.precision_recall(x, x[:2], k=3)
    with pytest.raises(ValueError):
        dm.knn_radii(x, 5)
    # and the library itself refuses what the wrapper would not pass on
    ws = torch.empty(4096, dtype=torch.float64, device="cuda")
    out = torch.empty(16, dtype=torch.float64, device="cuda")
    lib, ctx = B.lib(), B.get_ctx(x.device)
    assert lib.gi_feat_knn_radius(ctx, B.ptr(x), 5, 8, 5, B.ptr(ws), ws.numel() * 8, B.ptr(out)) != 0 and b"k=5" in lib.gi_last_error()
    assert lib.gi_feat_knn_radius(ctx, B.ptr(x), 5, 8, 0, B.ptr(ws), ws.numel() * 8, B.ptr(out)) != 0
    assert lib.gi_feat_knn_radius(ctx, B.ptr(x), 5, 0, 2, B.ptr(ws), ws.numel() * 8, B.ptr(out)) != 0
    assert lib.gi_feat_knn_radius(ctx, B.ptr(x), 5, 8, 2, B.ptr(ws), 8, B.ptr(out)) != 0 and b"workspace" in lib.gi_last_error()
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert lib.gi_kid_subset_sums(ctx, B.ptr(x), B.ptr(x), B.ptr(idx), B.ptr(idx), 1, 1, 8, B.ptr(ws), ws.numel() * 8, B.ptr(out)) != 0
    assert lib.gi_kid_subset_sums(ctx, B.ptr(x), B.ptr(x), B.ptr(idx), B.ptr(idx), 1, 2, 8193, B.ptr(ws), ws.numel() * 8, B.ptr(out)) != 0
    assert lib.gi_featmetrics_workspace_bytes(dm.WS_KID, 130, 0, 3) == 8 * 3 * 3 * 9
    assert lib.gi_featmetrics_workspace_bytes(dm.WS_RADIUS, 130, 0, 70) == 8 * (130 + 130 * 3 * 64)
    assert lib.gi_featmetrics_workspace_bytes(dm.WS_MEMBERS, 130, 33, 0) == 8 * 163


def test_results_are_reproducible_and_the_store_ignores_chunking():
    _, dm = _dm()
    real, fake = pr_inputs(130, 33, 64, 10)
    tr, tf = torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda()
    ix, iy = _lists(1, 130, 30), _lists(2, 33, 30)
    assert torch.equal(dm.kid_subset_sums(tr, tf, ix, iy), dm.kid_subset_sums(tr, tf, ix, iy))
    assert torch.equal(dm.knn_radii(tr, 3), dm.knn_radii(tr, 3))
    assert dm.kernel_inception_distance(tr, tf, 4, 20, 1) == dm.kernel_inception_distance(tr, tf, 4, 20, 1)
    whole = dm.FeatureStore("cuda", 64)
    whole.update(tr)
    parts = dm.FeatureStore("cuda", 64)
    for chunk in (tr[:1], tr[1:4], tr[4:]):
        parts.update(chunk)
    assert parts.count == 130 and torch.equal(parts.features(), whole.features()) and parts.features().is_contiguous()
    assert dm.kernel_inception_distance(parts, tf, 4, 20, 1) == dm.kernel_inception_distance(whole, tf, 4, 20, 1)
    assert dm.precision_recall(parts, tf) == dm.precision_recall(tr, tf)
    capped = dm.FeatureStore("cuda", 64, max_rows=50)
    for chunk in (tr[:30], tr[30:70], tr[70:]):
        capped.update(chunk)
    assert capped.count == 50 and torch.equal(capped.features(), tr[:50])


@pytest.fixture(scope="module")
def params():
    import inception_ref as R
    from util_golden import load
    return R.make_params(int(load("fid_inception")["param_seed"]))


def test_calculate_metric_with_dist_metrics(params):
    from test_fid_gpu import _FixedNet, _eval_batches
    _, dm = _dm()
    from gan_inpainting_amd.lib.fid import inception
    from gan_inpainting_amd.lib.models import evaluate
    model = inception.InceptionV3([3], dtype="fp16", max_batch=4)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model = model.cuda()
    batches, gens = _eval_batches()
    truth = np.random.Generator(np.random.PCG64(5)).random((12, 2048))
    fid_stats = (truth.mean(axis=0), np.cov(truth, rowvar=False))
    store = dm.FeatureStore("cuda", 2048)
    store.update(torch.from_numpy(truth.astype(np.float32)).cuda())
    cap = {}
    opts = {"kid_subsets": 4, "kid_subset_size": 5, "pr_k": 3, "seed": 2}
    met = evaluate.calculate_metric(torch.device("cuda"), batches, _FixedNet(gens), fid_stats=fid_stats, inception_model=model, epoch=1,
                                    fid_capture=cap, real_features=store, dist_metrics=("kid", "pr"), dist_options=opts)
    feats = cap["features"]
    assert tuple(feats.shape) == (6, 2048)
    assert set(met) == {"recon_rmse_global", "recon_l1_global", "recon_rmse_local", "recon_l1_local", "fid", "epoch", "kid", "precision", "recall"}
    assert met["kid"] == dm.kernel_inception_distance(store, feats, num_subsets=4, max_subset_size=5, seed=2)
    assert (met["precision"], met["recall"]) == dm.precision_recall(store, feats, k=3)
    assert all(isinstance(met[k], float) and np.isfinite(met[k]) for k in ("kid", "precision", "recall"))
    only = evaluate.calculate_metric(torch.device("cuda"), batches, _FixedNet(gens), inception_model=model, real_features=store,
                                     dist_metrics=("kid",), dist_options=opts)
    assert only["kid"] == met["kid"] and only["fid"] == -1 and "precision" not in only
    plain = evaluate.calculate_metric(torch.device("cuda"), batches, _FixedNet(gens), fid_stats=fid_stats, inception_model=model, epoch=1)
    assert set(plain) == {"recon_rmse_global", "recon_l1_global", "recon_rmse_local", "recon_l1_local", "fid", "epoch"}
    assert plain["fid"] == met["fid"]


@pytest.mark.parametrize("ema", [False, True])
def test_plugin_writes_kid_precision_recall(tmp_path, params, ema):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import train
    wpath = str(tmp_path / "pt_inception_standin.pth")
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd["fc.weight"], sd["fc.bias"] = torch.zeros(8, 2048), torch.zeros(8)
    torch.save(sd, wpath)
    train.main(["-exp", "minimaxgan_l1", "-ep", "1", "-b", "4", "--imagedim", "64", "--saveevery", "1", "--evalevery", "1",
                "--samples", "16", "--outdir", str(tmp_path), "--dtype", "fp16", "--fid-weights", wpath,
                "--dist-metrics", "kid,pr", "--pr-k", "3"] + (["--ema-decay", "0.9"] if ema else []))
    with open(os.path.join(str(tmp_path), "model", "minimaxgan_l1", "eval_history.obj"), "rb") as h:
        ev = pickle.load(h)
    assert set(ev[-1]) == ({"train", "test", "train_ema", "test_ema"} if ema else {"train", "test"})
    for part in ev[-1].values():
        for key in ("kid", "precision", "recall"):
            assert isinstance(part[key], float) and np.isfinite(part[key])
        assert 0.0 <= part["precision"] <= 1.0 and 0.0 <= part["recall"] <= 1.0
