"""Differentiable augmentation of the critic's inputs (Zhao et al. 2020, not in the reference): a random colour
change, translation and cutout per sample, applied to every image a discriminator sees, with the generator's gradient passing
through the transform's adjoint. Both directions are HIP kernels (csrc/diffaug.hip); the parameters are a pure function of
(policy, seed, step, call, row), so a run is reproducible and a resumed one replays the same transforms.

    aug = DiffAugment("color,translation,cutout", seed=0)
    d_pred_fake = D(aug(inpainted, step, 2))        # plugin-style code: autograd carries the adjoint
"""
import torch
from torch import nn

from ... import backend as B

POLICY_BITS = {"color": 1, "translation": 2, "cutout": 4}
CALL_REAL, CALL_FAKE, CALL_G = 0, 1, 2      # the critic update's real / generated half, the generator update's critic call

# how often each library entry was called through this module (tests: a step without the option never gets here)
CALLS = {"gi_diffaug_params": 0, "gi_diffaug_apply": 0, "gi_diffaug_apply_bwd": 0}


def parse_policy(policy):
    """'color,translation,cutout' (any non-empty subset, any order) -> the library's bit set. Raises ValueError otherwise."""
    names = [s.strip() for s in str(policy).split(",")]
    bits = 0
    for name in names:
        if name not in POLICY_BITS:
            raise ValueError(f"diffaug policy {policy!r}: {name!r} is not one of {', '.join(POLICY_BITS)}")
        bits |= POLICY_BITS[name]
    return bits


def key0(step, call, row0=0):
    """Key of the sample in row `row0`; the rows after it take the keys after it."""
    if not 0 <= int(call) <= 3 or int(step) < 0 or not 0 <= int(row0) < 1 << 32:
        raise ValueError(f"diffaug key: step {step}, call {call}, row {row0}")
    return (((int(step) * 4 + int(call)) << 32) | int(row0)) & 0xFFFFFFFFFFFFFFFF


def _check(x):
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 4 or x.shape[1] != 1:
        raise B.BackendError(f"DiffAugment takes (N,1,H,W) float32 images on the gfx950 device, got {tuple(x.shape)} {x.dtype} on {x.device}")
    if not x.is_contiguous():
        raise B.BackendError("DiffAugment takes contiguous images (a row slice of a larger batch is one)")


def apply_into(bits, seed, k0, x, out):
    """out = T(x) for the n rows of x (production entry: the parameters are drawn in the kernels)."""
    _check(x), _check(out)
    n, _, h, w = x.shape
    CALLS["gi_diffaug_apply"] += 1
    B.check(B.lib().gi_diffaug_apply(B.get_ctx(x.device), bits, seed, k0, B.ptr(x), n, h, w, B.ptr(out)))


def adjoint_into(bits, seed, k0, dy, out):
    """out = T*(dy): the gradient with respect to the un-augmented images."""
    _check(dy), _check(out)
    n, _, h, w = dy.shape
    CALLS["gi_diffaug_apply_bwd"] += 1
    B.check(B.lib().gi_diffaug_apply_bwd(B.get_ctx(dy.device), bits, seed, k0, B.ptr(dy), n, h, w, B.ptr(out)))


class _DiffAugFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bits, seed, k0):
        x = x.contiguous()
        y = torch.empty_like(x)
        apply_into(bits, seed, k0, x, y)
        ctx.args = (bits, seed, k0)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        adjoint_into(*ctx.args, dy, dx)
        return dx, None, None, None


class DiffAugment(nn.Module):
    """policy: 'color', 'translation', 'cutout' or any comma-separated subset. forward(x, step, call, row0=0) returns T(x) for
    the batch `step` (a counter the caller owns), the call site `call` (0 real half, 1 generated half of the critic update,
    2 the critic call of the generator update) and the batch rows row0 .. row0 + N - 1 (data parallel: rank * N). It has no
    parameters, buffers or state."""

    def __init__(self, policy, seed=0):
        super().__init__()
        self.bits = parse_policy(policy)
        self.policy = ",".join(k for k, b in POLICY_BITS.items() if self.bits & b)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def extra_repr(self):
        return f"policy={self.policy!r}, seed={self.seed}"

    def forward(self, x, step, call, row0=0):
        return _DiffAugFn.apply(x, self.bits, self.seed, key0(step, call, row0))

    def into(self, x, out, step, call, row0=0):
        """T(x) written into `out` (no autograd graph): the trainer's pair buffers."""
        apply_into(self.bits, self.seed, key0(step, call, row0), x, out)

    def adjoint_into(self, dy, out, step, call, row0=0):
        adjoint_into(self.bits, self.seed, key0(step, call, row0), dy, out)

    def params(self, step, call, n, H, W, row0=0, device=None):
        """The (n, 8) int32 parameter table of those samples on the device: b, c (fp32 bit patterns), ty, tx, y0, x0, ch, cw
        (view(torch.float32) of the first two columns gives b and c)."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        table = torch.empty((n, 8), dtype=torch.int32, device=dev)
        CALLS["gi_diffaug_params"] += 1
        B.check(B.lib().gi_diffaug_params(B.get_ctx(dev), self.bits, self.seed, key0(step, call, row0), n, H, W, B.ptr(table)))
        return table
