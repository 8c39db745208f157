"""Drop-in for the numeric part of the reference's lib/models/evaluate.py on fused HIP reductions:

  calculate_metric(device, loader, net, ...)            evaluate.py:85-177 (reconstruction metrics :127-158)
  calculate_segmentation_eval_metric(labels, outputs, unique_labels)     evaluate.py:179-224

The reference file does not import (mixed indentation, undefined `l1_criterion` / `segment`); what is
mirrored is what its plugins rely on (minimaxgan_l1.py:236-237: a dict with recon_rmse_global,
recon_l1_global, recon_rmse_local, recon_l1_local, fid, epoch). Out of this backend's scope and
reported as such: the matplotlib panels (`from_model_object`, `from_saved_obj`). FID (:155-163) is opt-in:
with `fid_stats` and an `inception_model` (lib.fid.inception.InceptionV3, weights loaded from a local file)
the pass feeds the composites the reference saves per image to the Inception handle and the fp64 device
statistic; without them `fid` is -1, the reference's own "not computed" value (:160). The reference writes
the composites as JPEG files and reads them back; here they keep the 8-bit truncation of
`(x * 255).astype(uint8)` but skip the file round trip (and with it JPEG's lossy coding).
Beside FID, opt-in (`dist_metrics`, `real_features`): the Kernel Inception Distance and improved precision / recall of the same
composites' features against stored ground-truth features (lib.fid.dist_metrics; the reference has neither).
Also opt-in (`lpips_model`, lib.lpips.LPIPS): the learned perceptual distance between composite and ground truth (csrc/lpips.hip).
Like the reference, calculate_metric does NOT switch the network to eval(): BatchNorm and Dropout run
in whatever mode the caller left them (training mode in the plugins)."""
import ctypes as C

import torch

from ... import backend as B


class ReconMeter:
    """Running sums of the four reconstruction metrics on the device (one readback at the end)."""

    def __init__(self, device):
        self.acc = torch.zeros(5, dtype=torch.float32, device=device)
        self._scratch = None

    def update(self, ground, gen, mask_c, want_output=False):
        """ground, gen, mask_c: (n,1,H,W) fp32 on the device; mask_c already ceil-ed / flipped."""
        n = ground.numel()
        lib, ctx = B.lib(), B.get_ctx(ground.device)
        ns = lib.gi_eval_recon_scratch_floats(n)
        if self._scratch is None or self._scratch.numel() * 2 < ns:
            self._scratch = torch.empty((ns + 1) // 2, dtype=torch.float64, device=ground.device)
        out = torch.empty_like(ground) if want_output else None
        B.check(lib.gi_eval_recon(ctx, B.ptr(ground), B.ptr(gen), B.ptr(mask_c), n, 1e-16, B.ptr(out), B.ptr(self.acc), None,
                                  B.ptr(self._scratch)))
        return out

    def result(self):
        a = self.acc.tolist()
        nb = max(a[4], 1.0)
        return {"recon_rmse_global": a[0] / nb, "recon_l1_global": a[1] / nb,
                "recon_rmse_local": a[2] / nb, "recon_l1_local": a[3] / nb}


@torch.no_grad()
def calculate_metric(device, loader, net, fid_stats=(-1, -1), mode="test", inception_model=None, epoch=None,
                     is_flip_mask=False, prepare=None, fid_capture=None, real_features=None, dist_metrics=(), dist_options=None,
                     panel=None, lpips_model=None):
    """evaluate.py:85-177. `loader` yields (input, mask, _) like the reference's datasets; `prepare` (optional)
    maps a loader item to a (n,1,h,w) float32 device tensor (the device Resize + ToTensor for decoded bytes).
    `fid_capture` (optional dict, tests): receives the composites fed to Inception and the pass's (mu, sigma).
    `dist_metrics`: names of lib.fid.dist_metrics.NAMES; with an `inception_model` and `real_features` (a FeatureStore or a
    (n,2048) device tensor of ground-truth features) the composites' features are kept as well (at most
    dist_options["max_images"] rows) and the record gains `kid` and / or `precision`, `recall` (dist_options: kid_subsets,
    kid_subset_size, pr_k, seed); fid_capture then also receives "features". Without them the record is what it always was.
    `panel` (optional, (path, K[, gutter])): the first K rows of the FIRST batch - ground | input | output | composite - are written
    to `path` as one greyscale PNG (lib.imageout.assemble_panel; K is clipped to the batch). It reuses the tensors of the pass: no
    extra forward, no random draw, so the metrics and everything that follows are what they are without it.
    `lpips_model` (optional, lib.lpips.LPIPS): every batch's composite (out * m + masked, NOT truncated to 8 bits) is compared with its
    ground truth; the per-image distances are summed on the device and read back once, and the record gains `lpips`, their mean.
    Without it the record and every launch are what they are without the argument."""
    lib = B.lib()
    meter = ReconMeter(device)
    fid_on = inception_model is not None and not _no_fid_stats(fid_stats)
    dist_on = bool(dist_metrics) and inception_model is not None and real_features is not None
    stats = store = None
    lpips_sum, lpips_count = None, 0
    if fid_on or dist_on:
        from ..fid import fid_score
    if fid_on:
        stats = fid_score.FidStats(inception_model.flat.device, 2048)
    if dist_on:
        from ..fid import dist_metrics as dm
        store = dm.FeatureStore(inception_model.flat.device, 2048, max_rows=(dist_options or {}).get("max_images"))
    for inp, mask, *_ in loader:
        if prepare is not None:
            inp, mask = prepare(inp), prepare(mask)     # images first: a prepare that generates masks sizes them like the batch's images
        else:
            inp = inp.to(device, non_blocking=True).float().contiguous()
            mask = mask.to(device, non_blocking=True).float().contiguous()
        m = torch.empty_like(mask)
        masked = torch.empty_like(inp)
        B.check(lib.gi_mask_apply(B.get_ctx(inp.device), B.ptr(inp), B.ptr(mask), B.ptr(m), B.ptr(masked), inp.numel(),
                                  1 | (2 if is_flip_mask else 0)))                  # :128-133
        out = net(masked)                                                            # :134
        out = out.detach().contiguous()
        meter.update(inp, out, m)                                                    # :135-143
        if panel is not None:
            _write_panel(panel, inp, masked, out, m)
            panel = None
        if lpips_model is not None or fid_on or dist_on:
            comp = torch.empty_like(out)                                             # :136 out * m + masked
            B.check(lib.gi_mask_composite(B.get_ctx(out.device), B.ptr(masked), B.ptr(out), B.ptr(m), B.ptr(comp), out.numel()))
        if lpips_model is not None:                                                  # the composite as it is, not truncated to 8 bits
            d = lpips_model.distance(comp, inp).sum()
            lpips_sum = d if lpips_sum is None else lpips_sum + d
            lpips_count += inp.shape[0]
        if fid_on or dist_on:
            comp = fid_score.quantize8(comp)                                         # :155-158 without the file (a new tensor)
            feats = inception_model.features(comp)
            if fid_on:
                stats.update(feats)
            if dist_on:
                store.update(feats)
            if fid_capture is not None:
                fid_capture.setdefault("composites", []).append(comp.cpu())
    metric = meter.result()
    fid = -1                                                                         # :160
    if fid_on:
        mu, sigma = stats.finish()
        fid = fid_score.calculate_frechet_distance(fid_stats[0], fid_stats[1], mu, sigma)   # :161-163
        if fid_capture is not None:
            fid_capture.update(mu=mu, sigma=sigma)
    metric.update({"fid": fid, "epoch": epoch})
    if dist_on:
        metric.update(dm.evaluate(real_features, store, dist_metrics, dist_options))
        if fid_capture is not None:
            fid_capture["features"] = store.features()
    if lpips_model is not None:
        metric["lpips"] = float(lpips_sum) / lpips_count if lpips_count else float("nan")
    return metric


def _write_panel(panel, inp, masked, out, m):
    """The sample panel of calculate_metric: K rows of ground | input | output | composite (masked + out * m)."""
    from .. import imageout
    path, k = panel[0], max(1, min(int(panel[1]), inp.shape[0]))
    cols = [t[:k].contiguous() for t in (inp, masked, out, m)]
    comp = torch.empty_like(cols[2])
    B.check(B.lib().gi_mask_composite(B.get_ctx(comp.device), B.ptr(cols[1]), B.ptr(cols[2]), B.ptr(cols[3]), B.ptr(comp), comp.numel()))
    imageout.write_png(path, imageout.assemble_panel(cols[:3] + [comp], gutter=int(panel[2]) if len(panel) > 2 else 2))


def _no_fid_stats(fid_stats):
    """The reference's `fid_stats[0] == -1 and fid_stats[1] == -1` (:161); None counts as not computed too."""
    if fid_stats is None or isinstance(fid_stats, (int, float)):
        return True
    return all(s is None or (not hasattr(s, "shape") and s == -1) for s in (fid_stats[0], fid_stats[1]))


def calculate_segmentation_eval_metric(labels, outputs, unique_labels):
    """evaluate.py:179-224. labels: (n,...) int64, outputs: (n,num_classes,...) fp32 logits, both on the
    device. Returns ({u: {'precision','recall','iou'}}, {'precision','recall','iou'}) of 0-d tensors."""
    if not labels.is_cuda or not outputs.is_cuda:
        raise B.BackendError("segmentation metrics take tensors on the gfx950 device")
    if labels.dtype != torch.int64 or outputs.dtype != torch.float32:
        raise B.BackendError("segmentation metrics take int64 labels and float32 logits")
    n, k = outputs.shape[0], outputs.shape[1]
    labels, outputs = labels.detach().contiguous(), outputs.detach().contiguous()
    hw = outputs.numel() // (n * k)
    if labels.numel() != n * hw:
        raise ValueError("labels %s do not match outputs %s" % (tuple(labels.shape), tuple(outputs.shape)))
    uniq = [int(u) for u in unique_labels]
    lib, ctx = B.lib(), B.get_ctx(outputs.device)
    per = torch.empty(len(uniq) * 3, dtype=torch.float32, device=outputs.device)
    across = torch.empty(3, dtype=torch.float32, device=outputs.device)
    counts = torch.empty(n * 16 * 3, dtype=torch.int32, device=outputs.device)
    hu = (C.c_int * len(uniq))(*uniq)
    B.check(lib.gi_seg_metrics(ctx, B.ptr(labels), B.ptr(outputs), n, k, hw, C.cast(hu, C.c_void_p), len(uniq), B.ptr(per),
                               B.ptr(across), B.ptr(counts)))
    names = ("precision", "recall", "iou")
    metric = {u: {nm: per[i * 3 + j] for j, nm in enumerate(names)} for i, u in enumerate(uniq)}
    return metric, {nm: across[j] for j, nm in enumerate(names)}
