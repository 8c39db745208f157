"""Distribution metrics on the pool3 features beside FID, computed on the device in fp64 (csrc/featmetrics.hip):

  FeatureStore(device, dims, max_rows)                  the feature rows of a pass, in arrival order
  kernel_inception_distance(real, fake, ...)            Binkowski et al. 2018: unbiased MMD^2, kernel (x.y / d + 1)^3
  precision_recall(real, fake, k)                       Kynkaanniemi et al. 2019: k-NN manifold membership

The reference project has neither; the definitions are restated in numpy fp64 in tests/featmetrics_ref.py. Only the index lists
of the KID subsets are made on the host (np.random.RandomState(seed): that order is part of the contract); every sum, distance,
radius and membership test runs on the device, and every result is the same bits run to run."""
import numpy as np
import torch

from ... import backend as B

WS_KID, WS_RADIUS, WS_MEMBERS = 0, 1, 2      # GI_FEAT_WS_* (include/ganinpaint.h)
NAMES = ("kid", "pr")


def parse_names(spec):
    """'kid,pr' -> ('kid', 'pr'); any non-empty subset, each name once."""
    names = tuple(s.strip() for s in str(spec).split(",") if s.strip())
    if not names or any(n not in NAMES for n in names) or len(set(names)) != len(names):
        raise ValueError("--dist-metrics takes a non-empty subset of %s (got %r)" % (",".join(NAMES), spec))
    return names


class FeatureStore:
    """Feature rows in arrival order up to max_rows; later rows are dropped. What it holds does not depend on how the rows were
    split into update() calls."""

    def __init__(self, device, dims=2048, max_rows=None):
        self.device = torch.device(device)
        self.dims = int(dims)
        self.max_rows = None if max_rows is None else int(max_rows)
        if self.max_rows is not None and self.max_rows < 0:
            raise ValueError("max_rows must not be negative (got %d)" % self.max_rows)
        self._chunks = []
        self.count = 0

    def update(self, feats):
        if not feats.is_cuda or feats.dtype != torch.float32 or feats.dim() != 2 or feats.shape[1] != self.dims:
            raise B.BackendError("FeatureStore.update takes (n,%d) float32 features on the gfx950 device" % self.dims)
        room = feats.shape[0] if self.max_rows is None else min(feats.shape[0], self.max_rows - self.count)
        if room <= 0:
            return
        self._chunks.append(feats[:room].detach().clone())
        self.count += room

    def features(self):
        """One contiguous (n, dims) float32 device tensor."""
        if not self._chunks:
            return torch.empty(0, self.dims, dtype=torch.float32, device=self.device)
        if len(self._chunks) > 1:
            self._chunks = [torch.cat(self._chunks)]
        return self._chunks[0]


def _features(x, what):
    if isinstance(x, FeatureStore):
        x = x.features()
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise B.BackendError("%s: (n,d) float32 features on the gfx950 device, or a FeatureStore" % what)
    return x.contiguous()


def _pair(real, fake, what):
    real, fake = _features(real, what), _features(fake, what)
    if real.shape[1] != fake.shape[1] or real.device != fake.device:
        raise ValueError("%s: real %s and fake %s features differ in width or device" % (what, tuple(real.shape), tuple(fake.shape)))
    return real, fake


def _workspace(op, n, n2, count, device):
    nbytes = B.lib().gi_featmetrics_workspace_bytes(op, n, n2, count)
    if nbytes < 0:
        raise B.BackendError("featmetrics: no workspace for op=%d n=%d n2=%d count=%d" % (op, n, n2, count))
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device), nbytes


def draw_subsets(seed, n_real, n_fake, m, num_subsets):
    """(real_idx, fake_idx), each (num_subsets, m) int32: per subset in turn m rows of the fake set, then m rows of the real set,
    each without replacement from np.random.RandomState(seed)."""
    rs = np.random.RandomState(seed)
    ir = np.empty((num_subsets, m), dtype=np.int32)
    jf = np.empty((num_subsets, m), dtype=np.int32)
    for s in range(num_subsets):
        jf[s] = rs.choice(n_fake, m, replace=False)
        ir[s] = rs.choice(n_real, m, replace=False)
    return ir, jf


def kid_subset_sums(real, fake, real_idx, fake_idx):
    """(num_subsets, 3) float64 on the device: { sum_{i != j} k(r_i, r_j), sum_{i != j} k(f_i, f_j), sum_{i,j} k(r_i, f_j) } over the
    rows the (num_subsets, m) index lists name. The lists are checked here; the library trusts them."""
    real, fake = _pair(real, fake, "kid_subset_sums")
    ir = np.ascontiguousarray(real_idx, dtype=np.int64)
    jf = np.ascontiguousarray(fake_idx, dtype=np.int64)
    if ir.ndim != 2 or ir.shape != jf.shape:
        raise ValueError("kid_subset_sums: index lists of shape (num_subsets, m) each (got %s, %s)" % (ir.shape, jf.shape))
    if ir.size and (ir.min() < 0 or ir.max() >= real.shape[0] or jf.min() < 0 or jf.max() >= fake.shape[0]):
        raise ValueError("kid_subset_sums: an index is outside its feature matrix")
    ns, m = ir.shape
    dev = real.device
    ix = torch.from_numpy(ir.astype(np.int32)).to(dev)
    iy = torch.from_numpy(jf.astype(np.int32)).to(dev)
    ws, nbytes = _workspace(WS_KID, m, 0, ns, dev)
    sums = torch.empty(ns, 3, dtype=torch.float64, device=dev)
    B.check(B.lib().gi_kid_subset_sums(B.get_ctx(dev), B.ptr(real), B.ptr(fake), B.ptr(ix), B.ptr(iy), ns, m, real.shape[1],
                                       B.ptr(ws), nbytes, B.ptr(sums)))
    return sums


def kernel_inception_distance(real, fake, num_subsets=100, max_subset_size=1000, seed=0):
    """mean over subsets of Sxx / (m (m-1)) + Syy / (m (m-1)) - 2 Sxy / m^2, m = min(n_real, n_fake, max_subset_size). When
    m == n_real == n_fake every subset is the whole of both sets: one subset over the rows in stored order, no draw."""
    real, fake = _pair(real, fake, "kernel_inception_distance")
    m = min(real.shape[0], fake.shape[0], int(max_subset_size))
    if m < 2:
        raise ValueError("KID needs at least 2 rows per set and subset (got %d real, %d fake, max_subset_size %d)"
                         % (real.shape[0], fake.shape[0], max_subset_size))
    if int(num_subsets) < 1:
        raise ValueError("KID needs at least one subset (got %d)" % num_subsets)
    if m == real.shape[0] == fake.shape[0]:
        ir = jf = np.arange(m, dtype=np.int32)[None]
    else:
        ir, jf = draw_subsets(seed, real.shape[0], fake.shape[0], m, int(num_subsets))
    s = kid_subset_sums(real, fake, ir, jf).cpu().numpy()
    terms = s[:, 0] / (m * (m - 1)) + s[:, 1] / (m * (m - 1)) - 2.0 * s[:, 2] / (m * m)
    return float(np.mean(terms))


def knn_radii(feats, k=3):
    """(n,) float64 on the device: squared distance of every row to its k-th nearest other row."""
    feats = _features(feats, "knn_radii")
    n, d = feats.shape
    k = int(k)
    if k < 1 or n <= k:
        raise ValueError("k-NN radii need 1 <= k < n (k=%d, n=%d)" % (k, n))
    ws, nbytes = _workspace(WS_RADIUS, n, 0, k, feats.device)
    radii = torch.empty(n, dtype=torch.float64, device=feats.device)
    B.check(B.lib().gi_feat_knn_radius(B.get_ctx(feats.device), B.ptr(feats), n, d, k, B.ptr(ws), nbytes, B.ptr(radii)))
    return radii


def manifold_members(ref, radii, probe):
    """(member, count): member (n_probe,) uint8 on the device, 1 where the probe row lies within radii[i] of some row i of ref;
    count a 0-d int32 device tensor."""
    ref, probe = _pair(ref, probe, "manifold_members")
    if radii.dtype != torch.float64 or radii.numel() != ref.shape[0] or radii.device != ref.device:
        raise ValueError("manifold_members: one float64 radius per reference row on the same device")
    radii = radii.contiguous()
    dev = ref.device
    ws, nbytes = _workspace(WS_MEMBERS, ref.shape[0], probe.shape[0], 0, dev)
    member = torch.empty(probe.shape[0], dtype=torch.uint8, device=dev)
    count = torch.empty((), dtype=torch.int32, device=dev)
    B.check(B.lib().gi_feat_manifold_members(B.get_ctx(dev), B.ptr(ref), ref.shape[0], B.ptr(radii), B.ptr(probe), probe.shape[0],
                                             ref.shape[1], B.ptr(ws), nbytes, B.ptr(member), B.ptr(count)))
    return member, count


def precision_recall(real, fake, k=3):
    """(precision, recall): the share of fake rows inside the real manifold, the share of real rows inside the fake one."""
    real, fake = _pair(real, fake, "precision_recall")
    k = int(k)
    if k < 1 or real.shape[0] <= k or fake.shape[0] <= k:
        raise ValueError("precision / recall with k=%d need more than k rows in both sets (got %d real, %d fake)"
                         % (k, real.shape[0], fake.shape[0]))
    _, in_real = manifold_members(real, knn_radii(real, k), fake)
    _, in_fake = manifold_members(fake, knn_radii(fake, k), real)
    return int(in_real) / fake.shape[0], int(in_fake) / real.shape[0]


def evaluate(real, fake, names, options=None):
    """The record entries of the evaluation pass: {'kid'} and / or {'precision', 'recall'} as Python floats."""
    o = dict(options or {})
    unknown = [n for n in names if n not in NAMES]
    if unknown:
        raise ValueError("unknown distribution metric(s) %r (known: %s)" % (unknown, ",".join(NAMES)))
    out = {}
    if "kid" in names:
        out["kid"] = kernel_inception_distance(real, fake, num_subsets=o.get("kid_subsets", 100),
                                               max_subset_size=o.get("kid_subset_size", 1000), seed=o.get("seed", 0))
    if "pr" in names:
        out["precision"], out["recall"] = precision_recall(real, fake, k=o.get("pr_k", 3))
    return out
