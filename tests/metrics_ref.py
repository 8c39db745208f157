"""Float64 restatements of the metric and auxiliary-loss kernels (csrc/ssim.hip, csrc/evalmetrics.hip, csrc/auxloss.hip), NumPy and
torch on the CPU. tests/test_metrics_ref_cpu.py proves them against torch and the oracle; tests/test_metric_ops_gpu.py compares the
kernels with them, per tile, per count and per gradient element instead of per mean.

  ssim_map / ssim_tiles   the SSIM map for ANY 1-D window (cross-correlation, as F.conv2d) and its sums per kernel tile
  ssim_probe              y = x except on a strip or a pixel next to a tile border: the neighbour tile sees the change through its halo only
  recon                   gi_eval_recon: the composite with the kernel's two fp32 roundings, the five sums in float64, the four metrics
  seg_counts / seg_ratios gi_seg_metrics: integer (|p & g|, |p|, |g|) with torch.argmax's rule, the ratios in the kernel's fp32 order
  tv / ce                 loss and full gradient by float64 autograd on oracle.torch_ref.tv_loss / F.cross_entropy"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_ref as orc

C1, C2 = 0.01 ** 2, 0.03 ** 2

# (shape, window) of the strip probes: one per tile kernel (ssim11_kernel, ssim_tile_kernel<16,64>, ssim_tile_kernel<8,32>)
PROBE_CASES = [((1, 1, 33, 129), 11), ((1, 1, 33, 129), 7), ((1, 1, 17, 65), 21)]
PROBE_KINDS = ("cols", "rows", "corner_in", "corner_out", "last")


def tile_of(ws):
    """(th, tw) of the kernel that serves window ws (ssim_plan of csrc/ssim.hip)."""
    return (16, 64) if ws <= 11 else (8, 32)


def gaussian(ws):
    """The metric's own window (fp32, as the reference builds it)."""
    return orc.ssim_window(ws)


def asymmetric_window(ws, seed):
    """A normalised random positive fp32 window that is no palindrome: g[k] != g[ws-1-k] for every k but the centre."""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = (0.2 + rng.random(ws)) * np.linspace(1.0, 3.0, ws)
    g = (g / g.sum()).astype(np.float32)
    assert ws == 1 or all(g[k] != g[ws - 1 - k] for k in range(ws // 2))
    return torch.from_numpy(g)


def ssim_map(x, y, g, dtype=torch.float64):
    """(n,c,H,W) SSIM map of x and y under the 1-D window g: five zero-padded depthwise cross-correlations with outer(g, g), evaluated in
    `dtype` (float64: the reference; float32: the yardstick of what fp32 arithmetic can give)."""
    x, y = torch.as_tensor(x).to(dtype), torch.as_tensor(y).to(dtype)
    g = torch.as_tensor(g).to(dtype)
    ws, c = g.numel(), x.shape[1]
    win = torch.outer(g, g)[None, None].expand(c, 1, ws, ws).contiguous()
    conv = lambda t: F.conv2d(t, win, padding=ws // 2, groups=c)
    mu1, mu2 = conv(x), conv(y)
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(x * x) - m11, conv(y * y) - m22, conv(x * y) - m12
    return ((2 * m12 + C1) * (2 * s12 + C2)) / ((m11 + m22 + C1) * (s1 + s2 + C2))


def ssim_tiles(m, th, tw):
    """sums [n*c, ty, tx] of the map over the kernel's th x tw tiles (partial[plane*tiles + ty*tx_count + tx] order, in the map's dtype)
    and pixels [ty, tx], the number of image pixels in each tile."""
    n, c, H, W = m.shape
    ty, tx = -(-H // th), -(-W // tw)
    pad = F.pad(m.reshape(n * c, H, W), (0, tx * tw - W, 0, ty * th - H))
    sums = pad.reshape(n * c, ty, th, tx, tw).sum(dim=(2, 4))
    ones = F.pad(torch.ones(H, W, dtype=torch.float64), (0, tx * tw - W, 0, ty * th - H))
    return sums, ones.reshape(ty, th, tx, tw).sum(dim=(1, 3))


def ssim_probe(x, kind, th, tw, r, seed=7):
    """(y, region): y = x except on `region` = (y0, y1, x0, x1), where fresh uniform noise stands:
    cols        the r columns left of the first vertical tile border, every row
    rows        the (at most r) rows above the first horizontal tile border, every column
    corner_in   the pixel (th-1, tw-1), the last of tile (0, 0)
    corner_out  the pixel (th, tw), the first of tile (1, 1)
    last        the pixel (H-1, W-1)"""
    H, W = x.shape[2:]
    region = {"cols": (0, H, tw - r, tw), "rows": (max(th - r, 0), th, 0, W), "corner_in": (th - 1, th, tw - 1, tw),
              "corner_out": (th, th + 1, tw, tw + 1), "last": (H - 1, H, W - 1, W)}[kind]
    y0, y1, x0, x1 = region
    assert 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W
    rng = np.random.Generator(np.random.PCG64(seed))
    y = np.array(x, dtype=np.float32, copy=True)
    y[:, :, y0:y1, x0:x1] = rng.random(y[:, :, y0:y1, x0:x1].shape, dtype=np.float32)
    return y, region


def probe_reach(region, r, H, W, th, tw):
    """bool [ty, tx]: the tiles with a pixel whose window touches the region (everywhere else the map is exactly 1)."""
    y0, y1, x0, x1 = region
    ty, tx = -(-H // th), -(-W // tw)
    lo_y, hi_y, lo_x, hi_x = max(y0 - r, 0), min(y1 + r, H) - 1, max(x0 - r, 0), min(x1 + r, W) - 1
    reach = np.zeros((ty, tx), dtype=bool)
    reach[lo_y // th: hi_y // th + 1, lo_x // tw: hi_x // tw + 1] = True
    return reach


def probe_corner(kind, H, W, th, tw):
    """The four tiles that share the tile corner the probe sits at, as (rows, cols) of tile indices."""
    if kind == "last":
        return ((H - 1) // th - 1, (H - 1) // th), ((W - 1) // tw - 1, (W - 1) // tw)
    return (0, 1), (0, 1)


def recon(ground, gen, m, eps):
    """gi_eval_recon on flat fp32 arrays: out = fl(fl(gen*m) + fl(ground*fl(1-m))) in fp32, bit for bit; sums = float64 [sum|d|, sum d^2,
    sum|dl|, sum dl^2, count(m != 0)] with d = fl(ground - out) and dl = fl(fl(out*m) - fl(ground*m)); metrics = fp32 [rmse_global,
    l1_global, rmse_local, l1_local] as eval_recon_final_kernel forms them (an empty mask gives 0/0 = nan for the local two)."""
    ground, gen, m = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (ground, gen, m))
    one = np.float32(1)
    out = (gen * m) + (ground * (one - m))
    assert out.dtype == np.float32
    d = (ground - out).astype(np.float64)
    dl = ((out * m) - (ground * m)).astype(np.float64)
    sums = np.array([np.abs(d).sum(), (d * d).sum(), np.abs(dl).sum(), (dl * dl).sum(), float(np.count_nonzero(m))], dtype=np.float64)
    count, e = float(ground.size), np.float64(np.float32(eps))
    with np.errstate(invalid="ignore", divide="ignore"):
        metrics = np.array([np.sqrt(sums[1] / count + e), sums[0] / count, np.sqrt(sums[3] / sums[4] + e), sums[2] / sums[4]]).astype(np.float32)
    return out, sums, metrics


def argmax_first(logits):
    """torch.argmax over axis 1 of (n, K, hw), restated: the first index of the maximum; NaN counts as the maximum, the first NaN wins."""
    lg = np.asarray(logits)
    best, arg = lg[:, 0].copy(), np.zeros(lg[:, 0].shape, dtype=np.int64)
    for k in range(1, lg.shape[1]):
        v = lg[:, k]
        with np.errstate(invalid="ignore"):
            take = (v > best) | (np.isnan(v) & ~np.isnan(best))
        best, arg = np.where(take, v, best), np.where(take, k, arg)
    return arg


def seg_counts(labels, logits, uniq):
    """int64 [n][nu][3] = (|p & g|, |p|, |g|), p = (argmax == u), g = (label == u) | (label == -1). labels (n, hw), logits (n, K, hw)."""
    labels = np.asarray(labels).reshape(len(labels), -1)
    arg = argmax_first(np.asarray(logits).reshape(labels.shape[0], -1, labels.shape[1]))
    out = np.zeros((labels.shape[0], len(uniq), 3), dtype=np.int64)
    for i, u in enumerate(uniq):
        p, g = arg == u, (labels == u) | (labels == -1)
        out[:, i] = np.stack([(p & g).sum(1), p.sum(1), g.sum(1)], 1)
    return out


def seg_ratios(counts):
    """seg_final_kernel: per_class fp32 [nu][3] = batch means of (precision, recall, iou), eps 1e-32, summed over the samples in order;
    across fp32 [3] = their mean over the classes, summed in order."""
    f, eps = np.float32, np.float32(1e-32)
    n, nu = counts.shape[:2]
    per, acc = np.zeros((nu, 3), dtype=np.float32), [f(0), f(0), f(0)]
    for u in range(nu):
        s = [f(0), f(0), f(0)]
        for b in range(n):
            inter, pc, gc = (f(int(v)) for v in counts[b, u])
            uni = f(int(counts[b, u, 1] + counts[b, u, 2] - counts[b, u, 0]))
            s = [s[0] + inter / (pc + eps), s[1] + inter / (gc + eps), s[2] + inter / (uni + eps)]
        for j in range(3):
            per[u, j] = s[j] / f(n)
            acc[j] = acc[j] + per[u, j]
    return per, np.array([a / f(nu) for a in acc], dtype=np.float32)


def tv(x, weight):
    """(loss, gradient [planes, H, W]) of oracle.torch_ref.tv_loss on the (planes, H, W) image stack, float64 autograd."""
    t = torch.as_tensor(x).double()[None].clone().requires_grad_(True)
    loss = orc.tv_loss(t, weight)
    loss.backward()
    return float(loss.detach()), t.grad[0].numpy()


def ce(z, y, weight, ignore_index, dtype=torch.float64):
    """(loss, gradient, weight sum) of F.cross_entropy on logits (n, K, hw) and labels (n, hw), autograd in `dtype`. Labels outside [0, K)
    become ignore_index first: the kernel ignores them, torch would raise. weight sum = sum of weight[y] over the pixels that count."""
    z, y = torch.as_tensor(z), torch.as_tensor(y).clone()
    K = z.shape[1]
    y[(y < 0) | (y >= K)] = ignore_index
    w = None if weight is None else torch.as_tensor(np.asarray(weight, dtype=np.float32)).to(dtype)
    t = z.to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(t, y, weight=w, ignore_index=ignore_index)
    loss.backward()
    valid = y[y != ignore_index]
    wsum = float(valid.numel()) if w is None else float(w.double()[valid].sum())
    return float(loss.detach()), t.grad.double().numpy(), wsum
