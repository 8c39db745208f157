"""Full-state checkpoints of a training run (host only): the file run_epochs writes with --save-state and reads with --resume.

    save_state(path, payload)          path + ".tmp", then os.replace: a killed save leaves the previous file intact
    load_state(path)                   the payload, on the CPU
    check_compatible(saved, current)   raises CheckpointError naming the first key that differs, with both values
    compat_args(state, world, nets)    the arguments a resumed run must share with the run that wrote the file

The payload is a plain dict of Python numbers, strings, lists, dicts and CPU tensors (DESIGN.md lists its keys); nothing in
it needs this package to unpickle."""
import os

import torch

FORMAT_VERSION = 1
STATE_FILE = "last_state.pt"

# a run resumed with another value of one of these would not continue the run that was saved
MATCH_KEYS = ("imagedim", "batchsize", "dtype", "generator", "discriminator", "gp_lambda", "g_every", "masks", "mask_seed", "flip",
              "ema_decay", "perceptual_grad", "face_parsing")
_DEFAULTS = {"dtype": "fp16", "generator": "unet", "discriminator": "patchgan", "gp_lambda": 0.0, "g_every": 0, "masks": "files",
             "mask_seed": 0, "flip": False, "ema_decay": 0.0, "perceptual_grad": False, "face_parsing": "off"}


class CheckpointError(RuntimeError):
    pass


def compat_args(state, world, nets):
    """{key: value} of MATCH_KEYS from a plugin's state, the world size, and every network's parameter count (nets: name -> network)."""
    out = {k: state.get(k, _DEFAULTS.get(k)) for k in MATCH_KEYS}
    if state.get("diffaug"):      # only when the option is on: states written without it keep their keys
        from .lib.models.augment import parse_policy
        out["diffaug"] = int(parse_policy(state["diffaug"]))
        out["diffaug_seed"] = int(state.get("diffaug_seed") or 0)
    if state.get("lpips_model") is not None:      # --lpips-weights: the evaluation records of the resumed run carry `lpips` too
        out["lpips"] = 1
    if state.get("lpips_loss"):        # --lpips-loss: only when set, so states written without it keep their keys
        out["lpips_loss"] = float(state["lpips_loss"])
    out["world_size"] = int(world)
    for name, net in nets.items():
        out[f"params/{name}"] = int(sum(p.numel() for p in net.parameters()))
    return out


def check_compatible(saved_args, args):
    """Every key of either side must be on both with equal values. numepoch, saveevery, evalevery, outdir, workers, cache and
    cache_budget_gb are not among them: they may differ (a different --cache changes the batch order, though)."""
    for k in sorted(set(saved_args) | set(args)):
        if k not in saved_args or k not in args:
            raise CheckpointError(f"cannot resume: {k!r} is {'missing from the saved state' if k not in saved_args else 'not set in this run'} "
                                  f"(saved {saved_args.get(k)!r}, this run {args.get(k)!r})")
        if saved_args[k] != args[k]:
            raise CheckpointError(f"cannot resume: {k} differs (saved {saved_args[k]!r}, this run {args[k]!r})")


def rng_path(path, rank):
    """The file beside `path` that holds rank `rank`'s RNG states: last_state.pt -> last_state.rng3.pt."""
    root = path[:-len(".pt")] if path.endswith(".pt") else path
    return f"{root}.rng{int(rank)}.pt"


def save_state(path, payload):
    tmp = path + ".tmp"
    try:
        torch.save(payload, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):       # serialisation raised half-way: the previous `path` is untouched
            os.remove(tmp)


def load_state(path):
    payload = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(payload, dict) or "format_version" not in payload:
        raise CheckpointError(f"{path} is not a training state written by --save-state")
    if payload["format_version"] != FORMAT_VERSION:
        raise CheckpointError(f"{path}: format version {payload['format_version']!r}, this code reads version {FORMAT_VERSION}")
    return payload


def resolve(resume, exp_dir):
    """--resume PATH|auto -> the file to load, or None to start fresh (auto with no file in the experiment's directory)."""
    if not resume:
        return None
    if resume == "auto":
        path = os.path.join(exp_dir, STATE_FILE)
        return path if os.path.exists(path) else None
    if not os.path.exists(resume):
        raise CheckpointError(f"--resume {resume}: no such file")
    return resume
