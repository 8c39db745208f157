"""Numpy restatement of the batch gather (csrc/batchgather.hip), independent of the product: Python integers for
the flip bits on the hash of tests/maskgen_ref.py, numpy indexing for the gather. Shares no code with gan_inpainting_amd."""
import numpy as np

from maskgen_ref import draw, mix, stream_of  # noqa: F401  (mix: the hash both are defined on)

FLIP_TAG = 0x666C6970   # "flip"
SPLIT_IDS = {"train": 0, "test": 1, "extra": 2}


def flip_bit(seed, key):
    """draw 0 of the key's stream under seed ^ "flip", top bit: independent of the mask draws of the same key."""
    return draw(stream_of((seed & ((1 << 64) - 1)) ^ FLIP_TAG, int(key)), 0) >> 31


def flip_bits(seed, keys):
    return [flip_bit(seed, k) for k in keys]


def key_of(split, epoch, row):
    """(split_id << 56) | (epoch << 32) | row, the epoch counted for the training split only (lib/data/masks.py)."""
    return (SPLIT_IDS[split] << 56) | ((int(epoch) if split == "train" else 0) << 32) | int(row)


def gather(store, rows, out_kind, flip_keys=None, seed=0):
    """store (N,h,w) uint8, rows n ints -> (n,h,w): out_kind 0 float32 v / 255 (both float32, like the kernel), 1 int64, 2 uint8."""
    store = np.asarray(store)
    assert store.dtype == np.uint8 and store.ndim == 3
    imgs = []
    for i, r in enumerate(rows):
        img = store[int(r)]
        if flip_keys is not None and flip_bit(seed, flip_keys[i]):
            img = img[:, ::-1]
        imgs.append(img)
    out = np.stack(imgs)
    if out_kind == 0:
        return out.astype(np.float32) / np.float32(255)
    return out.astype(np.int64 if out_kind == 1 else np.uint8)
