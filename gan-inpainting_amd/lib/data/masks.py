"""Hole masks generated on the device (csrc/maskgen.hip) instead of decoded from files: rectangles with the
benchmark's distribution or free-form strokes, each a pure function of (kind, seed, key, H, W). The key names the sample
(`mask_key`), so a test image gets the same mask in every epoch, at every world size and in any shuffling order, and a
training image a new one per epoch. Not in the reference, whose masks are PNG files (lib/data/dataset.py:35-51)."""
import torch

from ... import backend as B

KINDS = {"rect": 0, "freeform": 1}
SPLITS = {"train": 0, "test": 1, "extra": 2}


def mask_key(split, epoch, row):
    """(split_id << 56) | (epoch << 32) | row. `row` is an int or an int64 tensor of row ids (the result is then a tensor).
    Only the training split uses the epoch: evaluation masks are the same in every epoch."""
    sid = SPLITS[split]
    ep = int(epoch) if split == "train" else 0
    if not 0 <= ep < (1 << 24):
        raise ValueError(f"epoch {ep} does not fit the key's 24 bits")
    if torch.is_tensor(row):
        if row.dtype != torch.int64:
            raise ValueError("row ids are int64")
        if row.numel() and (int(row.min()) < 0 or int(row.max()) >= (1 << 32)):
            raise ValueError("a row id does not fit the key's 32 bits")
        return row + ((sid << 56) | (ep << 32))
    if not 0 <= int(row) < (1 << 32):
        raise ValueError(f"row id {row} does not fit the key's 32 bits")
    return (sid << 56) | (ep << 32) | int(row)


def is_key_item(t):
    """A loader's mask item that holds row ids (datasets with masks="generated") rather than mask pixels."""
    return torch.is_tensor(t) and t.dtype == torch.int64 and t.dim() == 1


class DeviceMaskGenerator:
    """keys (n,) int64, on the host or the device -> (n,1,H,W) float32 of {0,1} on the device."""

    def __init__(self, kind, H, W, seed=0):
        if kind not in KINDS:
            raise ValueError(f"mask kind {kind!r} (rect or freeform)")
        self.kind, self.H, self.W, self.seed = kind, int(H), int(W), int(seed) & ((1 << 64) - 1)

    def __call__(self, keys, return_coverage=False):
        if not is_key_item(keys):
            raise B.BackendError("DeviceMaskGenerator takes a (n,) int64 tensor of keys")
        if not keys.is_cuda:
            B.get_ctx()   # raises without a gfx950 device: there is no host fallback
            keys = keys.to(torch.device("cuda", torch.cuda.current_device()))
        keys = keys.contiguous()
        n = keys.numel()
        out = torch.empty((n, 1, self.H, self.W), dtype=torch.float32, device=keys.device)
        cover = torch.empty(n, dtype=torch.int32, device=keys.device) if return_coverage else None
        B.check(B.lib().gi_mask_generate(B.get_ctx(keys.device), KINDS[self.kind], self.seed, B.ptr(keys), n, self.H, self.W,
                                         B.ptr(out), B.ptr(cover)))
        return (out, cover) if return_coverage else out
