"""Shared host logic of the experiment plugins: the epoch loop, logging, bookkeeping and
checkpoint cadence of the reference plugins (experiment_list/minimaxgan_l1.py:83-261 and siblings)
around a per-batch step object from gan_inpainting_amd.trainer.

Differences to the reference, all host-side and listed in DESIGN.md:
  * save directory / log file come from state['outdir'] (the reference hard-codes
    /home/s2125048/thesis/model/<title>/ and log/<title>.log, minimaxgan_l1.py:27,34);
  * losses are read back once per `logevery` batches instead of ~45 blocking .item() calls per batch;
  * the gradient-flow histogram (one .item() per tensor per batch, :180-182,:195-197) is one kernel +
    one copy per batch (util.GradFlow), accumulated on the device;
  * the evaluation pass (minimaxgan_l1.py:234-240) runs lib.models.evaluate.calculate_metric on the
    train and test loaders (reconstruction metrics on fused HIP reductions; FID when state['inception_model']
    and state['train_fid'] / state['test_fid'] are set (train.py --fid-weights), else -1; `lpips` when state['lpips_model'] is set
    (train.py --lpips-weights)); `state['eval_fn']`, if given, replaces it and is called with (net_G, loader, epoch);
  * opt-in (train.py --save-state / --resume / --ema-decay; none of it in the reference): the full training state in last_state.pt
    at epoch boundaries, resuming from it, and an averaged generator evaluated and saved next to the live one.
"""
import contextlib
import logging
import os
import pickle
import time

import torch

from .. import checkpoint, optim, trainer
from ..lib.models import evaluate, networks, util


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def setup(state, title):
    state = state.copy()
    state.update({"title": title})
    outdir = state.get("outdir") or os.path.join(os.getcwd(), "runs")
    exp_dir = os.path.join(outdir, "model", title)
    os.makedirs(exp_dir, exist_ok=True)
    os.makedirs(os.path.join(outdir, "log"), exist_ok=True)
    logger = logging.getLogger(title)
    if not logger.handlers:
        # data-parallel runs: rank 0 owns the log file (and the checkpoints / histories, run_epochs)
        h = logging.FileHandler(os.path.join(outdir, "log", f"{title}.log")) if _rank() == 0 else logging.NullHandler()
        h.setFormatter(logging.Formatter("%(asctime)s %(message)s"))
        logger.addHandler(h)
        logger.propagate = _rank() == 0
    logger.setLevel(logging.INFO)
    if not torch.cuda.is_available():
        raise RuntimeError("the HIP backend needs a gfx950 device (there is no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    logger.info("using device %s", device)
    return state, exp_dir, logger, device


def build_networks(state, device, n_disc=1, sigmoid=True):
    """The generator and n_disc discriminators of a plugin. -d chooses the discriminator of the minimax plugins
    (minimaxgan_*, experiment1_global_local_D: PatchGAN or DCGAN); the WGAN plugins (sigmoid=False) always build a
    PatchGAN critic, as the reference hard-codes it (wgan_l1.py:58). state['spectral_norm'] / state['sn_iterations']
    (train.py --spectral-norm, --sn-iterations): every PatchGAN built here is spectrally normalised."""
    size = state["imagedim"]
    dtype = state.get("dtype", "fp16")
    disc = state.get("discriminator", "patchgan")
    sn = dict(spectral_norm=True, n_power_iterations=int(state.get("sn_iterations") or 1)) if state.get("spectral_norm") else {}
    if sn and disc == "dcgan":
        raise ValueError("--spectral-norm normalises the PatchGAN critic only: it cannot be combined with -d dcgan")
    if state.get("generator", "unet") != "unet" or disc not in ("patchgan", "dcgan"):
        raise NotImplementedError("HIP backend accelerates -g unet with -d patchgan or -d dcgan (train.py:27-28)")
    if disc == "dcgan" and not sigmoid:
        logging.getLogger(state.get("title", __name__)).info(
            "-d dcgan ignored: this plugin builds a PatchGAN critic without sigmoid, as the reference does (wgan_l1.py:58)")
        disc = "patchgan"
    if disc == "dcgan" and size != 128:
        raise ValueError(f"-d dcgan needs --imagedim 128: DCGANDiscriminator's Linear(36864, 4096) reads the 1024 x 6 x 6 "
                         f"features of a 128x128 image, got --imagedim {size}")
    num_downs = state.get("num_downs", 7 if size >= 128 else 6)
    if num_downs == 7:
        G = networks.get_network("generator", "unet", dtype=dtype)
    else:
        G = networks.UnetGenerator(1, 1, num_downs, ngf=64, use_dropout="False", dtype=dtype)
    if disc == "dcgan":   # experiment1_global_local_D: global and local discriminator both (reference :115-116)
        Ds = [networks.DCGANDiscriminator(dtype=dtype).to(device) for _ in range(n_disc)]
    else:
        Ds = [networks.get_network("discriminator", "patchgan", sigmoid=sigmoid, image_size=size, dtype=dtype, **sn).to(device)
              for _ in range(n_disc)]
    return G.to(device), Ds


def to_device_images(t, device, state):
    """Loader item -> (n,1,h,w) float32 on the device. Decoded 8-bit images (lib.data.dataset with transform=None)
    go through the device Resize + ToTensor (train.py:69-72); float tensors are taken as they are."""
    t = t.to(device, non_blocking=True)
    if t.dtype == torch.uint8:
        tf = state.get("_device_transform")
        if tf is None:
            from ..lib.data.dataset import DeviceResizeToTensor
            tf = state["_device_transform"] = DeviceResizeToTensor(state["imagedim"])
        return tf(t if t.dim() == 3 else t.reshape(-1, t.shape[-2], t.shape[-1]))
    return t.float().contiguous()


def to_device_mask(item, like, device, state, split, epoch):
    """A loader's mask item -> (n,1,h,w) float32 on the device. Row ids (int64 (n,): datasets with masks="generated") become the masks
    of --masks rect / freeform (lib/data/masks.py), sized like the batch's images `like` and keyed by (split, epoch, row): the
    training split's change per epoch, every other split's do not. Mask pixels (float, uint8) take to_device_images."""
    from ..lib.data import masks as M
    if not M.is_key_item(item):
        return to_device_images(item, device, state)
    kind = state.get("masks", "files")
    if kind not in M.KINDS:
        raise ValueError(f"the loader yields row ids instead of masks, which needs --masks rect or freeform (got {kind!r})")
    h, w = int(like.shape[-2]), int(like.shape[-1])
    gens = state.setdefault("_mask_generators", {})
    gen = gens.get((h, w))
    if gen is None:
        gen = gens[(h, w)] = M.DeviceMaskGenerator(kind, h, w, state.get("mask_seed", 0))
    return gen(M.mask_key(split, epoch, item).to(device, non_blocking=True))


def eval_prepare(state, device, split, epoch):
    """The `prepare` of evaluate.calculate_metric for one loader: it is applied to the images, then to the mask item of the same batch."""
    last = {}

    def prep(t):
        from ..lib.data.masks import is_key_item
        if is_key_item(t):
            if "images" not in last:
                raise RuntimeError("eval_prepare: a batch's row ids arrived before its images (calculate_metric prepares the images first)")
            return to_device_mask(t, last.pop("images"), device, state, split, epoch)
        last["images"] = to_device_images(t, device, state)
        return last["images"]
    return prep


def _fid_stats(state, mode):
    """state["train_fid"] / state["test_fid"] (train.py:177-178), or the reference's "not computed" pair."""
    st = state.get(mode + "_fid")
    return (-1, -1) if st is None or isinstance(st, (int, float)) else st


def _dist_kwargs(state, mode):
    """The opt-in arguments of evaluate.calculate_metric for KID / precision / recall (train.py --dist-metrics); {} when off."""
    names = state.get("dist_metric_names")
    feats = state.get(mode + "_feats")
    if not names or feats is None:
        return {}
    return {"real_features": feats, "dist_metrics": names, "dist_options": state.get("dist_options")}


def _panel_kwargs(state, mode, epoch, rank0, suffix=""):
    """The opt-in `panel` argument of evaluate.calculate_metric (train.py --sample-rows K): <outdir>/samples/<mode>_epoch<N>[_ema].png,
    written by rank 0; {} when off."""
    rows = int(state.get("sample_rows") or 0)
    if rows <= 0 or not rank0:
        return {}
    outdir = state.get("outdir") or os.path.join(os.getcwd(), "runs")
    return {"panel": (os.path.join(outdir, "samples", f"{mode}_epoch{epoch:04d}{suffix}.png"), rows, int(state.get("sample_gutter", 2)))}


def _lpips_kwargs(state):
    """The opt-in `lpips_model` argument of evaluate.calculate_metric (train.py --lpips-weights); {} when off."""
    model = state.get("lpips_model")
    return {} if model is None else {"lpips_model": model}


def _world():
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def make_ema(state, net_G):
    """optim.EMA of the generator when --ema-decay > 0, else None. Call it after the step object is built: its constructor
    broadcasts the parameters, so every replica's average starts from the same weights and needs no communication."""
    decay = float(state.get("ema_decay") or 0.0)
    return optim.EMA(net_G, decay) if decay > 0 else None


def lpips_loss_kw(state):
    """The opt-in LPIPS generator term of the WGAN steps (train.py --lpips-loss W): {lpips, lpips_weight} from state['lpips_model'] (the
    LPIPS(grad=True) object that also serves the metric) and state['lpips_loss']; {} when off."""
    w = float(state.get("lpips_loss") or 0.0)
    if not w:
        return {}
    model = state.get("lpips_model")
    if model is None or not getattr(model, "grad", False):
        raise ValueError("--lpips-loss needs --lpips-weights (an LPIPS(grad=True) model in state['lpips_model'])")
    return {"lpips": model, "lpips_weight": w}


def refuse_lpips_loss(state, name):
    """Plugins whose step has no oracle-pinned hook for an extra generator term."""
    if float(state.get("lpips_loss") or 0.0):
        raise ValueError(f"--lpips-loss is not defined for {name}: only the WGAN plugins (wgan_l1, wgan_rmse, "
                         "wgan_perceptual_style_faceparsing) take the term (DESIGN.md 4.13)")


def make_diffaug(state):
    """lib.models.augment.DiffAugment of state['diffaug'] / state['diffaug_seed'] (train.py --diffaug, --diffaug-seed), else None.
    Only the step object takes it: the evaluation passes, the averaged generator and FID never see an augmented image."""
    policy = state.get("diffaug")
    if not policy:
        return None
    from ..lib.models.augment import DiffAugment
    return DiffAugment(policy, seed=int(state.get("diffaug_seed") or 0))


def _rng_states(device):
    return {"torch": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(device)}


def _training_objects(net_G, nets_D, step):
    nets = {"G": net_G}
    nets.update({f"D{i}": d for i, d in enumerate(nets_D)})
    opts = {f"opt{i}": o for i, o in enumerate(getattr(step, "_opts", ()))}
    return nets, opts


def _save_training_state(path, state, epoch, history, eval_hist, counters, loaders, device, net_G, nets_D, step, rank0):
    """last_state.pt (rank 0) and this rank's RNG file. No collective: every rank reads its own objects."""
    torch.cuda.synchronize(device)        # the side stream's optimizer and its guard flags included
    rng = _rng_states(device)
    checkpoint.save_state(checkpoint.rng_path(path, _rank()), {"format_version": checkpoint.FORMAT_VERSION, "rank": _rank(), **rng})
    if not rank0:
        return
    nets, opts = _training_objects(net_G, nets_D, step)
    ema = getattr(step, "ema_G", None)
    payload = {
        "format_version": checkpoint.FORMAT_VERSION, "title": state["title"],
        "args": checkpoint.compat_args(state, _world(), nets), "epoch": int(epoch),
        "history": history, "eval_hist": eval_hist, "counters": dict(counters or {}),
        "nets": {k: {"state_dict": {n: v.detach().cpu().contiguous() for n, v in net.state_dict().items()},
                     "training_state": net.training_state()} for k, net in nets.items()},
        "optimizers": {k: o.state_dict() for k, o in opts.items()},
        "step": step.state_dict() if step is not None else None,
        "ema_G": ema.state_dict() if ema is not None else None,
        "loaders": {k: l.state_dict() for k, l in loaders.items() if l is not None and hasattr(l, "state_dict")},
        "rng": rng,
    }
    checkpoint.save_state(path, payload)


def _load_training_state(path, state, logger, counters, loaders, device, net_G, nets_D, step):
    """Restore everything _save_training_state wrote; returns (epoch, history, eval_hist). The RNG states go last: building
    the loaders, the FID statistics and the networks all drew from the generators before this point."""
    payload = checkpoint.load_state(path)
    if payload["title"] != state["title"]:
        raise checkpoint.CheckpointError(f"cannot resume: {path} was written by experiment {payload['title']!r}, this is {state['title']!r}")
    nets, opts = _training_objects(net_G, nets_D, step)
    checkpoint.check_compatible(payload["args"], checkpoint.compat_args(state, _world(), nets))
    for k, net in nets.items():
        net.load_state_dict(payload["nets"][k]["state_dict"])
        ts = dict(payload["nets"][k]["training_state"])
        if "dropout" in ts:    # the seed stays what the step constructor derived from the rank; the counter comes from the file
            ts["dropout"] = {"seed": net.training_state()["dropout"]["seed"], "counter": ts["dropout"]["counter"]}
        net.load_training_state(ts)
    if set(payload["optimizers"]) != set(opts):
        raise checkpoint.CheckpointError(f"cannot resume: the state holds optimizers {sorted(payload['optimizers'])}, this run {sorted(opts)}")
    for k, o in opts.items():
        o.load_state_dict(payload["optimizers"][k])
    if step is not None and payload.get("step") is not None:
        step.load_state_dict(payload["step"])
    ema = getattr(step, "ema_G", None)
    if (ema is None) != (payload.get("ema_G") is None):
        raise checkpoint.CheckpointError("cannot resume: the state and this run disagree on whether the generator is averaged (ema_decay)")
    if ema is not None:
        ema.load_state_dict(payload["ema_G"])
    for k, sd in payload.get("loaders", {}).items():
        if loaders.get(k) is not None and hasattr(loaders[k], "load_state_dict"):
            loaders[k].load_state_dict(sd)
    if counters is not None:
        counters.update(payload.get("counters", {}))
    rng_file = checkpoint.rng_path(path, _rank())
    rng = checkpoint.load_state(rng_file) if os.path.exists(rng_file) else payload["rng"]
    if not os.path.exists(rng_file) and _rank() != 0:
        raise checkpoint.CheckpointError(f"cannot resume: {rng_file} (this rank's RNG states) is missing")
    torch.cuda.synchronize(device)
    torch.set_rng_state(rng["torch"])
    torch.cuda.set_rng_state(rng["cuda"], device)
    logger.info("resumed from %s (epoch %d)", path, payload["epoch"])
    return int(payload["epoch"]), payload["history"], payload["eval_hist"]


def _g_state_dict(net_G):
    return {k: v.detach().cpu().contiguous() for k, v in net_G.state_dict().items()}


def run_epochs(state, loaders, exp_dir, logger, device, net_G, nets_D, batch_fn, d_names, pass_extra=False, step=None, counters=None):
    """batch_fn(batch_index, ground, mask[, extra]) -> (loss dict of device scalars, g_updated: bool); extra = the
    loader's third item (the segmentation labels of dataset.py:35-51) when pass_extra is set.
    counters: the plugin's dict of counters that outlive a batch (G_iter_count); saved and restored with the training state.
    state['save_state'] / state['state_every'] / state['resume'] (train.py --save-state, --state-every, --resume): DESIGN.md."""
    num_epochs, save_every, evaluate_every = state["numepoch"], state["saveevery"], state["evalevery"]
    log_every = state.get("logevery", 50)
    gscale = step.sync.grad_scale() if (step is not None and getattr(step, "sync", None) is not None) else 1.0
    flow_G = util.GradFlow(net_G, gscale)
    flows_D = [util.GradFlow(d, gscale) for d in nets_D]
    history, eval_hist = [], []
    side = step.side_stream() if step is not None else None
    side_keys = set(step.side_keys()) if step is not None else set()
    rank0 = _rank() == 0
    ema = getattr(step, "ema_G", None)
    state_every = int(state.get("state_every") or save_every)
    state_path = os.path.join(exp_dir, checkpoint.STATE_FILE)
    first_epoch = 0
    resume = checkpoint.resolve(state.get("resume"), exp_dir)
    if state.get("resume") and resume is None:
        logger.info("--resume auto: no %s, starting fresh", state_path)
    if resume is not None:
        done, history, eval_hist = _load_training_state(resume, state, logger, counters, loaders, device, net_G, nets_D, step)
        if done >= num_epochs:
            logger.info("%s holds epoch %d, -ep is %d: nothing left to train", resume, done, num_epochs)
            return history
        first_epoch = done + 1

    def _on(stream):
        return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()

    for epoch in range(first_epoch, num_epochs + 1):
        start = time.time()
        sums, g_updates, batches = {}, 0, 0
        acc_g = torch.zeros(len(flow_G.names), device=device)
        with _on(side):
            acc_d = [torch.zeros(len(f.names), device=device) for f in flows_D]
        train = loaders["train"]
        if state.get("flip") and hasattr(train, "augmented"):     # --flip: the cached loader's pass with this epoch's flips
            train = train.augmented(epoch)
        for bi, (ground, mask, extra) in enumerate(train):
            ground = to_device_images(ground, device, state)
            mask = to_device_mask(mask, ground, device, state, "train", epoch)
            if pass_extra:
                L, g_updated = batch_fn(bi, ground, mask, extra.to(device, non_blocking=True).contiguous())
            else:
                L, g_updated = batch_fn(bi, ground, mask)
            # values the step produced on its side stream (overlapped critic: its losses, its gradient buffer) are
            # accumulated ON that stream, in stream order behind the kernels that wrote them and ahead of the next
            # batch's zero_grad; everything else on the caller's stream. No cross-stream wait per batch.
            for k, v in L.items():
                with _on(side if k in side_keys else None):
                    if k not in sums:
                        sums[k] = torch.zeros(1, dtype=torch.float32, device=device)
                    sums[k] += v.detach().view(1)
            batches += 1
            with _on(side):
                for f, a in zip(flows_D, acc_d):
                    a += f.measure()
            if g_updated:
                g_updates += 1
                acc_g += flow_G.measure()
            if bi % log_every == 0:
                if step is not None:
                    step.poll_overflow(logger)                 # fp16 guard: back the loss scale off after skipped updates
                    step.sync_for_logging()                    # the values below may come from the side stream
                logger.info("[epoch %d/%d][batch %d/%d] %s", epoch, num_epochs, bi, len(loaders["train"]),
                            " ".join(f"{k}: {float(v):.4f}" for k, v in L.items()))
        if step is not None:
            step.sync_for_logging()
        rec = {k: float(v) / max(batches, 1) for k, v in sums.items()}
        grads = {"avg_g": dict(zip(flow_G.names, (acc_g / g_updates).tolist())) if g_updates
                 else {n: -7777 for n in flow_G.names}}     # -7777 sentinel: minimaxgan_l1.py:209-218
        for name, f, a in zip(d_names, flows_D, acc_d):
            grads[name] = dict(zip(f.names, (a / max(batches, 1)).tolist()))
        history.append({"losses": rec, "g_updates": g_updates, "gradients": grads})
        if epoch % evaluate_every == 0 and epoch > 0:
            if state.get("eval_fn"):
                eval_hist.append(state["eval_fn"](net_G, loaders.get("test"), epoch))
            else:                                                # minimaxgan_l1.py:235-240
                rec_eval = {k: evaluate.calculate_metric(device, loaders[k], net_G, fid_stats=_fid_stats(state, k), mode=k,
                                                         inception_model=state.get("inception_model"), epoch=epoch,
                                                         prepare=eval_prepare(state, device, k, epoch), **_dist_kwargs(state, k),
                                                         **_panel_kwargs(state, k, epoch, rank0), **_lpips_kwargs(state))
                            for k in ("train", "test") if loaders.get(k) is not None}
                if ema is not None:                              # the same metrics of the averaged generator
                    with ema.applied():
                        for k in ("train", "test"):
                            if loaders.get(k) is not None:
                                rec_eval[k + "_ema"] = evaluate.calculate_metric(
                                    device, loaders[k], net_G, fid_stats=_fid_stats(state, k), mode=k,
                                    inception_model=state.get("inception_model"), epoch=epoch, prepare=eval_prepare(state, device, k, epoch),
                                    **_dist_kwargs(state, k), **_panel_kwargs(state, k, epoch, rank0, "_ema"), **_lpips_kwargs(state))
                eval_hist.append(rec_eval)
                logger.info("VALIDATION: %s", ", ".join(f"{k} - {v}" for k, v in rec_eval.items()))
            if rank0:        # every rank holds the same replica: one writer
                with open(os.path.join(exp_dir, "training_epoch_history.obj"), "wb") as h:
                    pickle.dump(history, h, protocol=pickle.HIGHEST_PROTOCOL)
                with open(os.path.join(exp_dir, "eval_history.obj"), "wb") as h:
                    pickle.dump(eval_hist, h, protocol=pickle.HIGHEST_PROTOCOL)
        if epoch % save_every == 0 and epoch > 0 and rank0:
            # same contract as the reference: G only, plain state_dict (minimaxgan_l1.py:253-255)
            torch.save(_g_state_dict(net_G), os.path.join(exp_dir, "epoch{}_G.pt".format(epoch)))
            if ema is not None:     # the averaged weights under the same keys (BatchNorm statistics: the live ones)
                with ema.applied():
                    torch.save(_g_state_dict(net_G), os.path.join(exp_dir, "epoch{}_G_ema.pt".format(epoch)))
        if state.get("save_state") and epoch > 0 and epoch % state_every == 0:
            _save_training_state(state_path, state, epoch, history, eval_hist, counters, loaders, device, net_G, nets_D, step, rank0)
        logger.info("epoch: %d, time: %.3fs, %s", epoch, time.time() - start,
                    ", ".join(f"{k}: {v:.6f}" for k, v in rec.items()))
    return history


def make_optimizers(kind, net_G, d_params):
    if kind == "adam":    # minimaxgan_l1.py:64-65
        return (optim.Adam(net_G.parameters(), lr=0.0002, betas=(0.5, 0.999)),
                optim.Adam(d_params, lr=0.0002, betas=(0.5, 0.999)))
    return (optim.RMSprop(net_G.parameters(), lr=0.00005),     # wgan_l1.py:64-65
            optim.RMSprop(d_params, lr=0.00005))


def wgan_cadence(state, batch_index, g_iter_count):
    """Whether this batch updates the generator: the reference rule (wgan_l1.py:157-163: every 140th batch while
    fewer than 25 generator updates were made or their count is a multiple of 500, else every 5th; never batch 0),
    or, with --g-every N (an extension for short runs: the reference rule never fires in epochs shorter than 141
    batches), every Nth batch."""
    if state.get("g_every"):
        return batch_index % int(state["g_every"]) == 0 and batch_index > 0
    return trainer.wgan_update_g(batch_index, g_iter_count, update_g_every=5)


def make_sync():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        from .. import parallel
        return parallel.GradSync()
    return None


__all__ = ["setup", "build_networks", "run_epochs", "make_optimizers", "make_sync", "make_ema", "make_diffaug", "wgan_cadence", "trainer"]
