"""Drop-in for the numeric part of the reference's lib/fid/fid_score.py.

  calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps)   fid_score.py:128-179, host fp64, no scipy
  FidStats                                                    streaming mean / covariance in fp64 on the device
  calculate_activation_statistics(images, model, ...)         fid_score.py:182-204 over a loader or a tensor
  _compute_statistics_of_path(path, model, batch_size, dims, cuda)   fid_score.py:207-218 (folder of images or .npz)

The reference takes tr sqrtm(S1 S2) from scipy. The trace of the principal square root is the sum of the principal square
roots of the eigenvalues of S1 S2, which torch.linalg.eigvals gives in fp64 on the host; the real part is kept, as the
reference keeps the real part of its matrix. For covariance matrices the eigenvalues are real and non-negative up to
rounding; real parts below zero (rank-deficient products) are clamped at zero.

Where this differs from the reference on purpose: (1) the reference raises ValueError when the diagonal of its complex square
root has an imaginary part above 1e-3 (:169-174); the eigenvalue form has no such matrix: imaginary parts of eigenvalues are
dropped and negative real parts clamped without an error. (2) `quantize8` clamps to [0, 255] before the division, whereas
`(x * 255).astype(uint8)` wraps around for values outside [0, 1]; inside [0, 1], where images live, the two agree bit for bit."""
import pathlib

import numpy as np
import torch

from ... import backend as B
from .inception import InceptionV3  # noqa: F401  (the reference's module exposes it too)


def _trace_sqrt_product(sigma1, sigma2):
    """tr sqrtm(sigma1 @ sigma2) in fp64 (may be non-finite when the eigenvalue solver fails)."""
    prod = torch.from_numpy(np.ascontiguousarray(sigma1.dot(sigma2)))
    if not bool(torch.isfinite(prod).all()):
        return float("nan")
    try:
        ev = torch.linalg.eigvals(prod)
    except RuntimeError:
        return float("nan")
    re = torch.clamp(ev.real, min=0.0)
    return float(torch.sqrt(re).sum())


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = ||mu1 - mu2||^2 + Tr(S1 + S2 - 2 sqrt(S1 S2)), with the reference's fallback: when the first attempt at the
    square-root term is not finite, eps is added to the diagonals of both covariances and the term is taken again."""
    mu1 = np.atleast_1d(np.asarray(mu1, dtype=np.float64))
    mu2 = np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    sigma1 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64))
    sigma2 = np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"
    diff = mu1 - mu2
    tr_covmean = _trace_sqrt_product(sigma1, sigma2)
    if not np.isfinite(tr_covmean):
        print("fid calculation produces singular product; adding %s to diagonal of cov estimates" % eps)
        offset = np.eye(sigma1.shape[0]) * eps
        tr_covmean = _trace_sqrt_product(sigma1 + offset, sigma2 + offset)
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr_covmean)


class FidStats:
    """Sum and X^T X of feature rows in fp64 on the device (gi_fid_stats_*): every element is accumulated row by row in
    arrival order, so (mu, sigma) do not depend on how the loader was batched and two runs give the same bits."""

    def __init__(self, device, dims=2048):
        self.dims = int(dims)
        self.device = torch.device(device)
        self.acc = torch.zeros(B.lib().gi_fid_stats_acc_doubles(self.dims), dtype=torch.float64, device=self.device)
        self.count = 0

    def update(self, feats):
        if not feats.is_cuda or feats.dtype != torch.float32 or feats.dim() != 2 or feats.shape[1] != self.dims:
            raise B.BackendError("FidStats.update takes (n,%d) float32 features on the gfx950 device" % self.dims)
        feats = feats.contiguous()
        B.check(B.lib().gi_fid_stats_update(B.get_ctx(feats.device), B.ptr(self.acc), B.ptr(feats), feats.shape[0], self.dims))
        self.count += feats.shape[0]

    def finish_device(self):
        mu = torch.empty(self.dims, dtype=torch.float64, device=self.device)
        sigma = torch.empty(self.dims, self.dims, dtype=torch.float64, device=self.device)
        B.check(B.lib().gi_fid_stats_finish(B.get_ctx(self.device), B.ptr(self.acc), B.ptr(mu), B.ptr(sigma), self.dims))
        return mu, sigma

    def finish(self):
        """(mu, sigma) as numpy fp64, sigma with the n - 1 divisor of np.cov(rowvar=False)."""
        if self.count < 2:
            raise ValueError("FID statistics need at least 2 images (got %d)" % self.count)
        mu, sigma = self.finish_device()
        return mu.cpu().numpy(), sigma.cpu().numpy()


def quantize8(x):
    """What a picture becomes on its way through an 8-bit file: (x * 255).astype(uint8) / 255 (evaluate.py:156, fid_score.py:102-107)."""
    # a tensor divisor: dividing by a Python scalar multiplies by its rounded reciprocal on the device, the reference divides
    return torch.clamp(torch.floor(x * 255.0), 0.0, 255.0) / torch.full((), 255.0, dtype=x.dtype, device=x.device)


@torch.no_grad()
def calculate_activation_statistics(images, model, batch_size=50, dims=2048, cuda=True, verbose=False, quantize=False, store=None):
    """images: a (n,1|3,H,W) float tensor in [0,1], or an iterable of such tensors or of loader items whose first entry is
    one. Returns (mu, sigma) in fp64 from the device statistic. store (optional, lib.fid.dist_metrics.FeatureStore): is fed
    the same feature batches, so the rows themselves outlive the sweep; (mu, sigma) are the same with and without it."""
    if dims != 2048:
        raise NotImplementedError("only the 2048-wide pool3 features are built (dims=%r)" % (dims,))
    dev = model.flat.device
    stats = FidStats(dev, dims)
    if torch.is_tensor(images):
        images = [images[i:i + batch_size] for i in range(0, images.shape[0], batch_size)]
    for item in images:
        x = item[0] if isinstance(item, (tuple, list)) else item
        x = x.to(dev, non_blocking=True).float().contiguous()
        if quantize:
            x = quantize8(x)
        feats = model.features(x)
        stats.update(feats)
        if store is not None:
            store.update(feats)
    return stats.finish()


def imread(filename):
    """(height, width, 3) uint8, grey images replicated (fid_score.py:59-63 after grey2rgb)."""
    from PIL import Image
    a = np.asarray(Image.open(filename), dtype=np.uint8)
    if a.ndim == 2:
        a = np.repeat(a[..., None], 3, axis=2)
    return a[..., :3]


def _compute_statistics_of_path(path, model, batch_size, dims, cuda):
    path = str(path)
    if path.endswith(".npz"):
        with np.load(path) as f:
            return f["mu"][:], f["sigma"][:]
    p = pathlib.Path(path)
    files = sorted(list(p.glob("*.jpg")) + list(p.glob("*.png")))

    def batches():
        for i in range(0, len(files), batch_size):
            arr = np.array([imread(str(f)).astype(np.float32) for f in files[i:i + batch_size]]).transpose((0, 3, 1, 2)) / 255
            yield torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
    return calculate_activation_statistics(batches(), model, batch_size, dims, cuda)
