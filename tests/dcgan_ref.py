"""CPU helper for the DCGANDiscriminator tests, restated from the architecture (reference lib/models/networks.py:162-212):
4 x [Conv2d 5x5 s1 p1 + bias, ReLU, MaxPool 2/2], NCHW flatten, Linear 36864 -> 4096, ReLU, Linear 4096 -> 512, ReLU,
Linear 512 -> 2, Softmax(dim 1), view(-1, 1).

  * make_params(seed): a machine-independent weight set (numpy PCG64, fan-in-scaled uniform) under the reference's keys;
  * forward(P, x): the functional restatement in any torch dtype;
  * decision_aware(P, x, dy, hip, band): fp64 gradients with the HIP forward's decisions imposed where the two forwards
    may legitimately disagree (in the style of oracle/kink.py): ReLU inputs within `band` of zero and pool windows whose
    top two candidates are closer than `band`. Everywhere else the reference's decisions stand, and a HIP decision that
    differs there is counted in the returned `mismatch`.
"""
import numpy as np
import torch
import torch.nn.functional as F

CHANS = [1, 128, 256, 512, 1024]
LINEARS = ((12, 36864, 4096), (14, 4096, 512), (16, 512, 2))


def keys_and_shapes():
    out = []
    for i in range(4):
        out.append((f"model.{3 * i}.weight", (CHANS[i + 1], CHANS[i], 5, 5)))
        out.append((f"model.{3 * i}.bias", (CHANS[i + 1],)))
    for idx, fi, fo in LINEARS:
        out.append((f"model.{idx}.weight", (fo, fi)))
        out.append((f"model.{idx}.bias", (fo,)))
    return out


def make_params(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    P = {}
    for k, shape in keys_and_shapes():
        fan_in = int(np.prod(shape[1:])) if k.endswith("weight") else None
        if fan_in is None:   # bias: the fan-in of its weight
            fan_in = int(np.prod(P[k[:-len("bias")] + "weight"].shape[1:]))
        b = 1.0 / np.sqrt(fan_in)
        P[k] = rng.uniform(-b, b, size=shape).astype(np.float32)
    return P


def to_torch(P, dtype=torch.float64):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in P.items()}


def forward(T, x):
    """T: dict of tensors (one dtype), x: (N,1,128,128). Returns (2N, 1)."""
    a = x
    for i in range(4):
        a = F.max_pool2d(F.relu(F.conv2d(a, T[f"model.{3 * i}.weight"], T[f"model.{3 * i}.bias"], padding=1)), 2, 2)
    h = a.reshape(a.shape[0], -1)
    h = F.relu(F.linear(h, T["model.12.weight"], T["model.12.bias"]))
    h = F.relu(F.linear(h, T["model.14.weight"], T["model.14.bias"]))
    return torch.softmax(F.linear(h, T["model.16.weight"], T["model.16.bias"]), dim=1).reshape(-1, 1)


def _windows(z, hp):
    """(N,C,H,W) pre-activation -> (N,C,hp,hp,4) pool candidates in window order (0,0) (0,1) (1,0) (1,1)."""
    n, c = z.shape[:2]
    w = z[:, :, :2 * hp, :2 * hp].reshape(n, c, hp, 2, hp, 2)
    return w.permute(0, 1, 2, 4, 3, 5).reshape(n, c, hp, hp, 4)


def decision_aware(P, x, dy, hip, band):
    """fp64 forward + backward of sum(y * dy) with imposed decisions.
    hip: dict with 'dec1'..'dec4' (N,C,hp,hp) HIP pool decisions (sub-position + 4 if the winner was > 0), 'h12', 'h14'
         (N,F) HIP post-ReLU Linear activations (their sign is the HIP decision).
    band: dict with 'pool1'..'pool4', 'h12', 'h14' absolute bands.
    Returns (y, grads dict with 'x' and every parameter key, stats dict: imposed / mismatch counts and unit totals)."""
    T = {k: v.clone().requires_grad_(True) for k, v in to_torch(P).items()}
    xx = x.detach().to(torch.float64).clone().requires_grad_(True)
    stats = dict(imposed=0, mismatch=0, units=0)
    a = xx
    hps = [63, 30, 14, 6]
    for i in range(4):
        z = F.conv2d(a, T[f"model.{3 * i}.weight"], T[f"model.{3 * i}.bias"], padding=1)
        win = _windows(z, hps[i])
        with torch.no_grad():
            srt = win.sort(dim=-1, descending=True).values
            # reference decision: first maximum in window order, winner positive
            s_ref = (win == srt[..., :1]).to(torch.int64).argmax(dim=-1)
            pos_ref = srt[..., 0] > 0
            hd = hip[f"dec{i + 1}"].to(torch.int64)
            s_hip, pos_hip = hd & 3, (hd & 4) != 0
            risk = ((srt[..., 0] - srt[..., 1]) < band[f"pool{i + 1}"]) | (srt[..., 0].abs() < band[f"pool{i + 1}"])
            # a disagreement matters only where some side routes a gradient (its winner positive)
            differ = (pos_ref != pos_hip) | (pos_ref & (s_ref != s_hip))
            stats["mismatch"] += int((differ & ~risk).sum())
            stats["imposed"] += int((risk & differ).sum())
            stats["units"] += risk.numel()
            s = torch.where(risk, s_hip, s_ref)
            pos = torch.where(risk, pos_hip, pos_ref)
        a = win.gather(-1, s.unsqueeze(-1)).squeeze(-1) * pos.to(torch.float64)
    h = a.reshape(a.shape[0], -1)
    for idx, key in ((12, "h12"), (14, "h14")):
        pre = F.linear(h, T[f"model.{idx}.weight"], T[f"model.{idx}.bias"])
        with torch.no_grad():
            ref = pre > 0
            mine = hip[key].to(torch.float64) > 0
            risk = pre.abs() < band[key]
            stats["mismatch"] += int(((ref != mine) & ~risk).sum())
            stats["imposed"] += int(((ref != mine) & risk).sum())
            stats["units"] += pre.numel()
            keep = torch.where(risk, mine, ref)
        h = pre * keep.to(torch.float64)
    y = torch.softmax(F.linear(h, T["model.16.weight"], T["model.16.bias"]), dim=1).reshape(-1, 1)
    (y * dy.to(torch.float64)).sum().backward()
    grads = {k: v.grad for k, v in T.items()}
    grads["x"] = xx.grad
    return y.detach(), grads, stats


def pool_preacts(P, x, dtype=torch.float64):
    """Per conv layer: the pool candidates (N,C,hp,hp,4) of the reference forward (for measuring bands)."""
    T = to_torch(P, dtype)
    a = x.to(dtype)
    out = []
    for i, hp in enumerate([63, 30, 14, 6]):
        z = F.conv2d(a, T[f"model.{3 * i}.weight"], T[f"model.{3 * i}.bias"], padding=1)
        out.append(_windows(z, hp))
        a = F.max_pool2d(F.relu(z), 2, 2)
    h = a.reshape(a.shape[0], -1)
    h12 = F.linear(h, T["model.12.weight"], T["model.12.bias"])
    h14 = F.linear(F.relu(h12), T["model.14.weight"], T["model.14.bias"])
    return out, h12, h14
