"""Device-resident dataset cache (train.py --cache device): every file of a dataset is decoded and resized ONCE,
the 8-bit results of the Resize stay on the device, and every later batch - of a training epoch, an evaluation pass, the FID
ground-truth pass - is assembled by one gather kernel (csrc/batchgather.hip). A batch assembled on the device can flip its images
horizontally for free: `DeviceCachedLoader.augmented(epoch)` does, keyed like the generated masks (lib/data/masks.py) but on a
stream of its own. Not in the reference, which decodes every file again in every pass (lib/data/dataset.py:35-51)."""
import torch

from ... import backend as B
from . import masks as M
from .dataset import DeviceResizeToTensor

KINDS = ("ground", "mask", "segment")
OUT_F32, OUT_I64, OUT_U8 = 0, 1, 2
CHUNK = 32                    # images decoded, copied and resized per step of the build
_GOLDEN = 0x9E3779B97F4A7C15


class CacheBudgetError(RuntimeError):
    """The cache does not fit its memory budget."""


def cache_bytes(n, h, w, masks=False, segments=False):
    """Device bytes of the stores of n images resized to h x w: one byte per pixel and kind."""
    return int(n) * int(h) * int(w) * (1 + int(bool(masks)) + int(bool(segments)))


def check_budget(need, budget):
    if need > budget:
        raise CacheBudgetError(f"the device cache needs {need} bytes ({need / 2**30:.2f} GiB) and its budget is {budget} bytes "
                               f"({budget / 2**30:.2f} GiB): raise --cache-budget-gb, lower --imagedim or train with --cache off")


def epoch_order(n, seed, pass_index):
    """The order of pass `pass_index` over n rows: a permutation of 0..n-1, a pure function of (n, seed, pass_index)."""
    g = torch.Generator()
    g.manual_seed((int(seed) + _GOLDEN * (int(pass_index) + 1)) & ((1 << 63) - 1))
    return torch.randperm(int(n), generator=g)


def _collate(batch):
    """collate_fn of the build: the shapes of every sample (so that the first row whose size differs can be named) and, where the
    shapes agree, the stacked items - stacked in the worker, so one tensor per kind crosses the process boundary, not one per sample."""
    shapes = [tuple(tuple(t.shape) for t in sample) for sample in batch]
    same = all(sh == shapes[0] for sh in shapes)
    return shapes, tuple(torch.stack([sample[j] for sample in batch]) for j in range(3)) if same else None


def _check_rows(rows, n_store):
    """rows -> a non-empty 1-d int64 tensor with every entry in [0, n_store); one small sync when it lives on the device."""
    if not torch.is_tensor(rows):
        rows = torch.as_tensor(rows)
    if rows.dtype != torch.int64 or rows.dim() != 1 or rows.numel() == 0:
        raise ValueError("rows is a non-empty 1-d int64 tensor (or a list of ints)")
    lo, hi = torch.stack((rows.min(), rows.max())).tolist()
    if lo < 0 or hi >= n_store:
        raise IndexError(f"row {lo if lo < 0 else hi} is outside the cache's {n_store} images")
    return rows


class DeviceImageCache:
    """(N,h,w) uint8 stores on the device: the resized ground truths, the resized masks (masks="files") and the segment label maps
    (when the rows have them); `row_ids` are the dataset's `_row` ids, on the host."""

    def __init__(self, ground, mask, segment, row_ids):
        self.stores = {"ground": ground, "mask": mask, "segment": segment}
        self.row_ids = row_ids
        self.n, self.h, self.w = (int(s) for s in ground.shape)
        self.device = ground.device

    def __len__(self):
        return self.n

    @property
    def nbytes(self):
        return sum(s.numel() for s in self.stores.values() if s is not None)

    @classmethod
    def build(cls, dataset, size, device, workers=0, budget_bytes=None):
        """Runs `dataset` (an InpaintingDataset with transform=None) once, in order."""
        if getattr(dataset, "transform", None) is not None:
            raise ValueError("the cache takes a dataset with transform=None: the Resize runs on the device")
        device = torch.device(device)
        B.get_ctx(device)    # raises without a gfx950 device: there is no host fallback
        n = len(dataset)
        if n == 0:
            raise ValueError("the dataset is empty")
        with_masks = getattr(dataset, "masks", "files") == "files"
        df = getattr(dataset, "image_df", None)
        if df is not None and "_row" in df.columns:
            row_ids = torch.tensor([int(r) for r in df["_row"]], dtype=torch.int64)
        else:
            row_ids = torch.arange(n, dtype=torch.int64)
        # workers hand their chunks over in shared memory: pinned (train.py's loader settings), or the device copy of a large
        # chunk is slow
        kw = {"prefetch_factor": 4, "pin_memory": True} if int(workers) > 0 else {}
        loader = torch.utils.data.DataLoader(dataset, batch_size=CHUNK, shuffle=False, drop_last=False, num_workers=int(workers),
                                             collate_fn=_collate, **kw)
        tf = DeviceResizeToTensor(size)
        ground = mask = segment = None
        first = None              # the first row's item shapes: (ground, mask, segment)
        at = 0
        with torch.cuda.device(device):
            for shapes, items in loader:
                if first is None:
                    first = shapes[0]
                    with_segments = len(first[2]) == 2
                    h, w = tf.output_size(*first[0])
                    need = cache_bytes(n, h, w, with_masks, with_segments)
                    if budget_bytes is None:
                        budget_bytes = torch.cuda.mem_get_info(device)[0] // 2
                    check_budget(need, int(budget_bytes))
                    ground = torch.empty((n, h, w), dtype=torch.uint8, device=device)
                    mask = torch.empty((n, h, w), dtype=torch.uint8, device=device) if with_masks else None
                    segment = torch.empty((n, h, w), dtype=torch.uint8, device=device) if with_segments else None
                for i, (gs, ms, ss) in enumerate(shapes):
                    if gs != first[0] or ms != first[1]:
                        other = gs if gs != first[0] else ms
                        raise ValueError(f"row {at + i}: a source of {' x '.join(map(str, other))} where the rows before it have "
                                         f"{' x '.join(map(str, first[0]))} (all sources of one CSV share a size)")
                    if (len(ss) == 2) != with_segments:
                        raise ValueError(f"row {at + i}: {'a' if len(ss) == 2 else 'no'} segment map where the rows before it have "
                                         f"{'none' if len(ss) == 2 else 'one'}")
                    if with_segments and ss != (h, w):
                        raise ValueError(f"row {at + i}: a segment map of {ss} beside a resized image of {(h, w)}")
                g, m, s = items
                k = len(shapes)
                if with_segments:
                    flat = s.reshape(k, -1)
                    lo, hi = flat.amin(1), flat.amax(1)
                    bad = ((lo < 0) | (hi > 255)).nonzero()
                    if bad.numel():
                        i = int(bad[0])
                        raise ValueError(f"row {at + i}: segment labels {int(lo[i])} .. {int(hi[i])} outside 0 .. 255")
                    segment[at:at + k] = s.to(torch.uint8).to(device)
                ground[at:at + k] = tf(g.to(device), return_bytes=True)[:, 0]
                if with_masks:
                    mask[at:at + k] = tf(m.to(device), return_bytes=True)[:, 0]
                at += k
        if at != n:
            raise RuntimeError(f"the dataset yielded {at} of its {n} rows")
        return cls(ground, mask, segment, row_ids)

    def gather(self, rows, kind, flip_keys=None, flip_seed=0, raw=False):
        """Images `rows` (int64, host or device) of store `kind`, flipped where (flip_seed, flip_keys[i]) says (None: nowhere):
        "ground" / "mask" -> (n,1,h,w) float32 in [0,1], "segment" -> (n,h,w) int64; raw=True -> the stored bytes, (n,h,w) uint8.
        A fresh tensor per call, written asynchronously on the current stream."""
        if kind not in KINDS:
            raise ValueError(f"kind {kind!r} ({', '.join(KINDS)})")
        store = self.stores[kind]
        if store is None:
            raise ValueError(f"the cache holds no {kind} store")
        rows = _check_rows(rows, self.n).to(self.device).contiguous()
        if flip_keys is not None:
            if not M.is_key_item(flip_keys) or flip_keys.numel() != rows.numel():
                raise ValueError("flip_keys is a (n,) int64 tensor, one key per row")
            flip_keys = flip_keys.to(self.device).contiguous()
        return self._gather(rows, kind, flip_keys, flip_seed, raw)

    def _gather(self, rows, kind, flip_keys, flip_seed, raw=False):
        """gather() without the checks: rows and flip_keys are contiguous int64 tensors on the device, rows known to be in range."""
        store = self.stores[kind]
        n = rows.numel()
        if raw:
            code, out = OUT_U8, torch.empty((n, self.h, self.w), dtype=torch.uint8, device=self.device)
        elif kind == "segment":
            code, out = OUT_I64, torch.empty((n, self.h, self.w), dtype=torch.int64, device=self.device)
        else:
            code, out = OUT_F32, torch.empty((n, 1, self.h, self.w), dtype=torch.float32, device=self.device)
        B.check(B.lib().gi_batch_gather(B.get_ctx(self.device), B.ptr(store), self.n, self.h, self.w, B.ptr(rows), n,
                                        B.ptr(flip_keys), int(flip_seed) & ((1 << 64) - 1), code, B.ptr(out)))
        return out


class DeviceCachedLoader:
    """Batches of a DeviceImageCache in the shape the training and evaluation loops take from a DataLoader: (ground (n,1,h,w)
    float32 on the device, mask (n,1,h,w) float32 on the device - or the host int64 row ids when the masks are generated -,
    segment (n,h,w) int64 on the device - or the (n,1) zeros placeholder). drop_last, a fresh permutation per pass
    (`epoch_order` of the loader's seed and its pass count), fresh output tensors per batch. Plain iteration never flips."""

    def __init__(self, cache, batch_size, split, seed=None, flip_seed=0):
        if split not in M.SPLITS:
            raise ValueError(f"split {split!r} ({', '.join(M.SPLITS)})")
        if not 0 < int(batch_size) <= len(cache):
            raise ValueError(f"batch size {batch_size} with {len(cache)} cached rows")
        self.cache, self.batch_size, self.split = cache, int(batch_size), split
        # seed None: drawn from torch's global generator, so torch.manual_seed reproduces a run
        self.seed = int(torch.randint(0, 1 << 62, ()).item()) if seed is None else int(seed)
        self.flip_seed = int(flip_seed)
        self.passes = 0

    def __len__(self):
        return len(self.cache) // self.batch_size

    def state_dict(self):
        """(seed, passes): what the order of every later pass follows from (resumable training)."""
        return {"seed": int(self.seed), "passes": int(self.passes)}

    def load_state_dict(self, sd):
        self.seed, self.passes = int(sd["seed"]), int(sd["passes"])

    def __iter__(self):
        return self._batches(None)

    def augmented(self, epoch):
        """One pass like plain iteration, each ground truth and its segment map flipped horizontally where
        (flip_seed, mask_key(split, epoch, row)) says; masks do not flip."""
        return self._batches(int(epoch))

    def _batches(self, epoch):
        c, b = self.cache, self.batch_size
        order = epoch_order(len(c), self.seed, self.passes)
        self.passes += 1
        ids = c.row_ids[order]                        # host
        order_dev = order.to(c.device)
        keys_dev = None if epoch is None else M.mask_key(self.split, epoch, ids).to(c.device)
        for i in range(len(self)):
            rows = order_dev[i * b:(i + 1) * b]
            keys = None if keys_dev is None else keys_dev[i * b:(i + 1) * b]
            ground = c._gather(rows, "ground", keys, self.flip_seed)
            mask = c._gather(rows, "mask", None, 0) if c.stores["mask"] is not None else ids[i * b:(i + 1) * b].clone()
            if c.stores["segment"] is not None:
                segment = c._gather(rows, "segment", keys, self.flip_seed)
            else:
                segment = torch.zeros((b, 1), dtype=torch.int64)
            yield ground, mask, segment
