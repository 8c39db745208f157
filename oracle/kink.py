"""Kink-aware gradient references (test infrastructure, see oracle/__init__.py).

Why. The gradient tests compare whole gradient tensors of UnetGenerator / PatchGANDiscriminator
(lib/models/networks.py:216-363) at 1e-3 of max|ref| per tensor. Two correct fp32 evaluations of these graphs agree to
~1e-6 in the forward, but a ReLU / LeakyReLU input within that distance of zero can land on either side of its kink, and
with the tests' random-sign objective ONE such unit moves gradient tensors by 1e-3 .. 4e-1 of their max (measured unit by
unit with `flip_impacts` below: every single at-risk unit of a 64x64 case is worth more than 1e-3 somewhere). A case
with ~5e5 .. 3e7 activations has 0.3 .. 3 such units between ANY two fp32 evaluations, so no seed list can make a strict
comparison hold "by luck" on the larger sizes, and margins of 10 x the measured forward error exist on no seed at all
(counting argument in DESIGN.md section 2).

What is decidable from the oracle alone is WHERE a correct fp32 forward may disagree about a kink:
  eps(z)   = max |z32 - z64| over a tapped pre-activation tensor, the oracle's own fp32 forward error of that tensor;
  at risk  = |z64| < BAND * eps(z)  (never: exact zeros of both evaluations, and units removed by dropout).
The reference gradient of a case is then the fp64 oracle evaluated with, on the at-risk units ONLY, the side of the kink
the implementation under test actually took in its own forward (read back through gi_net_saved_activation; the value is
continuous there, only the derivative branch differs: torch_ref._act). Outside the band the oracle's own decisions
stand and the tests assert that the implementation took the same ones (a kink disagreement at |z| >= BAND * eps is a
wrong forward, not rounding). The comparison itself is strict on every tensor and runs on ONE fixed seed per case: no
retry, no seed chosen by looking at a result.

fp16 runs: the implementation's forward error is the half-precision one. What that error HAS to be comes from the oracle too:
torch_ref's storage-rounded restatement (store=store_fp16: fp64 arithmetic, every tensor the engine keeps in fp16 rounded where
the engine writes it) against the fp64 oracle gives eps16(z) = max |z16 - z64| per tapped tensor, and the band is
min(FP16_BAND * max|z64|, K * eps16(z)) - never wider than the constant it replaces. `yardstick` is the same restatement's error
on every tensor the tests compare (kink decisions inside the band taken from the restatement, as they are taken from the
implementation under test), and `fp16_parity` bounds an implementation by K times it.
"""
import numpy as np
import torch

from . import params as _p
from . import torch_ref as _o

BAND = 16.0          # fp32: at risk when |z64| < BAND * max|z32 - z64| (BAND * eps ~ 1e-5 of the tensor's largest value)
FP16_BAND = 2e-2     # fp16: at risk when |z64| < min(FP16_BAND * max|z64|, K * eps16)
K = 4.0              # fp16: an implementation may err K times as much as the storage-rounded restatement (tests/test_fid_gpu.py::_bound)
FLOOR32 = 1e-4       # ... plus what this suite allows the fp32 engine (fp32 bound of every parity test): between its stores the fp16
                     # engine computes in fp32 while the restatement computes in fp64, and some tensors have a yardstick of exactly
                     # zero (the critic's Linear bias gradient without sigmoid is sum(R), whatever the network computes)
BAND_SHARE_CAP = 5e-2   # fp16: at most this share of a case's live units may lie inside the band
FLIP_SHARE_CAP = 2e-3   # fp16: at most this share may actually be decided by the implementation

_CACHE = {}          # what the fp32 and fp16 runs of ONE case share (the case evaluated last)


def _cached(case, what, fn):
    key = case.get("key")
    if key is None:
        return fn()
    if _CACHE.get("key") != key:
        _CACHE.clear()
        _CACHE["key"] = key
    if what not in _CACHE:
        _CACHE[what] = fn()
    return _CACHE[what]


def unet_channels(nd, ngf=64):
    return [0] + [ngf * min(2 ** (k - 1), 8) for k in range(1, nd + 1)]


def unet_case(seed, nd, N, HW, norm="batch"):
    """Inputs of one generator parity case: weights, masked image, objective weights R (loss = sum(y * R)), dropout masks."""
    P = _p.make_unet_params(seed, num_downs=nd, ngf=64, norm=norm)
    ground, mask = _p.synth_batch(seed + 7, N, HW, HW)
    x = torch.from_numpy(ground * (1 - mask))
    R = torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(size=(N, 1, HW, HW), dtype=np.float32))
    masks = {k: torch.from_numpy(v) for k, v in _p.synth_dropout_masks(seed + 13, nd, N, HW, HW).items()}
    return {"kind": "unet", "P": P, "x": x, "R": R, "masks": masks, "nd": nd, "norm": norm, "N": N, "HW": HW,
            "key": ("unet", seed, nd, N, HW, norm)}


def patchgan_case(seed, HW, N, sigmoid, groups=1):
    """groups = 2: the N images are two consecutive BatchNorm populations of N / 2, i.e. two critic calls on the same parameters
    (wgan_l1.py:134-135 D(ground), D(inpainted)) whose gradients accumulate; the second half is shifted and scaled so that the
    two populations have different statistics."""
    P = _p.make_patchgan_params(seed, HW, HW)
    ground, _ = _p.synth_batch(seed + 3, N, HW, HW)
    if groups == 2:
        ground[N // 2:] = ground[N // 2:] * 0.5 + 0.2
    r = torch.from_numpy(np.random.Generator(np.random.PCG64(seed + 5)).standard_normal(size=(N, 1), dtype=np.float32))
    return {"kind": "patchgan", "P": P, "x": torch.from_numpy(ground), "R": r, "sigmoid": sigmoid, "N": N, "HW": HW, "groups": groups,
            "key": ("patchgan", seed, HW, N, sigmoid, groups)}


def tap_shapes(case):
    """{tap name: ((N,C,h,w), kind, level)}: the tensors that feed a kink and where gi_net_saved_activation keeps the
    activation behind each (generator: d<k> -> kind 0 level k; u<k> -> kind 1 level k-1; critic: c<i> -> kind 0 level i)."""
    N, HW = case["N"], case["HW"]
    out = {}
    if case["kind"] == "unet":
        nd = case["nd"]
        ch = unet_channels(nd)
        for k in range(1, nd + 1):
            out[f"d{k}"] = ((N, ch[k], HW >> k, HW >> k), 0, k)
        for k in range(2, nd + 1):
            out[f"u{k}"] = ((N, ch[k - 1], HW >> (k - 1), HW >> (k - 1)), 1, k - 1)
    else:
        for i, c in ((1, 64), (2, 128), (3, 256), (4, 512)):
            out[f"c{i}"] = ((N, c, HW >> i, HW >> i), 0, i)
    return out


def run(case, dtype, taps=None, flips=None, backward=True, store=None):
    """One oracle evaluation of loss = sum(y * R) -> (y, {name: parameter gradient}, input gradient, parameters).
    store: torch_ref.store_fp16 for the storage-rounded restatement (None: the oracle itself)."""
    OP = _o.to_torch(case["P"], dtype=dtype)
    x = case["x"].to(dtype).clone().requires_grad_(backward)
    with torch.set_grad_enabled(backward):
        if case["kind"] == "unet":
            y = _o.unet_forward(OP, x, case["nd"], True, case["masks"], norm=case["norm"], taps=taps, flips=flips, store=store)
        elif case.get("groups", 1) == 2:   # two calls, one per population, in the reference's order (running statistics move twice)
            h = case["N"] // 2
            ys, tt = [], [{}, {}]
            for g in range(2):
                fl = {k: v[g * h:(g + 1) * h] for k, v in flips.items()} if flips else None
                ys.append(_o.patchgan_forward(OP, x[g * h:(g + 1) * h], case["sigmoid"], True, taps=tt[g] if taps is not None else None, flips=fl, store=store))
            y = torch.cat(ys)
            if taps is not None:
                for k in tt[0]:
                    taps[k] = torch.cat([tt[0][k], tt[1][k]])
        else:
            y = _o.patchgan_forward(OP, x, case["sigmoid"], True, taps=taps, flips=flips, store=store)
        if backward:
            (y * case["R"].to(dtype)).sum().backward()
    grads = {k: OP[k].grad for k in _o.named_parameter_keys(case["P"])} if backward else None
    return y.detach(), grads, (x.grad if backward else None), OP


def _running(OP):
    return {k: v.detach() for k, v in OP.items() if k.endswith("running_mean") or k.endswith("running_var")}


def _forward(case, dtype):
    taps = {}
    y, _, _, OP = run(case, dtype, taps, None, backward=False)
    return {"y": y, "stats": _running(OP), "taps": {k: v.detach() for k, v in taps.items()}}


def forward32(case):
    """The oracle's fp32 forward (cached per case): dict(y, stats = running statistics after the forward, taps)."""
    return _cached(case, "f32", lambda: _forward(case, torch.float32))


def forward64(case):
    return _cached(case, "f64", lambda: _forward(case, torch.float64))


def restated(case):
    """The storage-rounded restatement (fp64 arithmetic, fp16 stores), forward and backward, cached per case:
    dict(y, stats, taps, grads, dx)."""
    def go():
        taps = {}
        y, g, dx, OP = run(case, torch.float64, taps, None, backward=True, store=_o.store_fp16)
        return {"y": y, "stats": _running(OP), "taps": {k: v.detach() for k, v in taps.items()}, "grads": g, "dx": dx}
    return _cached(case, "r16", go)


def eps16(case):
    """{tap: max |z16 - z64|}: the forward error fp16 storage has to cost on each tapped tensor."""
    def go():
        t16, t64 = restated(case)["taps"], forward64(case)["taps"]
        return {k: float((t16[k] - t64[k]).abs().max()) for k in t64 if not k.endswith(".keep")}
    return _cached(case, "eps16", go)


def survey(case, band=BAND, fp16=False):
    """The oracle's two forwards with taps -> {tap: dict(z64, live, at_risk, eps)} (no gradients)."""
    t32, t64 = forward32(case)["taps"], forward64(case)["taps"]
    e16 = eps16(case) if fp16 else None
    out = {}
    for name, z64 in t64.items():
        if name.endswith(".keep"):
            continue
        z32 = t32[name].double()
        eps = float((z32 - z64).abs().max())
        live = ~((z64 == 0) & (z32 == 0))
        if name + ".keep" in t64:
            live &= t64[name + ".keep"].bool()
        width = min(FP16_BAND * float(z64.abs().max()), K * e16[name]) if fp16 else band * eps
        out[name] = {"z64": z64, "live": live, "eps": eps, "width": width, "at_risk": live & (z64.abs() < width)}
    return out


def kink_reference(case, decisions, band=BAND, fp16=False):
    """decisions: {tap: bool tensor (N,C,h,w), True where the implementation's saved activation is > 0}.
    -> (y64, grads64, dx64, report): the fp64 oracle with the implementation's decisions on the at-risk units; report
    counts the at-risk units, the decisions taken from the implementation and the disagreements OUTSIDE the band (with
    the largest |z64| / width among them), which a correct forward does not have."""
    sv = survey(case, band, fp16)
    flips, rep = {}, {"units": 0, "at_risk": 0, "flipped": 0, "outside": 0, "outside_worst": 0.0, "eps": {}}
    for name, s in sv.items():
        dec = decisions[name].to(s["z64"].device)
        disagree = (dec != (s["z64"] > 0)) & s["live"]
        inside = disagree & s["at_risk"]
        outside = disagree & ~s["at_risk"]
        rep["units"] += int(s["live"].sum())
        rep["at_risk"] += int(s["at_risk"].sum())
        rep["flipped"] += int(inside.sum())
        rep["eps"][name] = s["eps"]
        if outside.any():
            rep["outside"] += int(outside.sum())
            rep["outside_worst"] = max(rep["outside_worst"], float(s["z64"].abs()[outside].max()) / max(s["width"], 1e-300))
        if inside.any():
            flips[name] = inside
    y, g, dx, _ = run(case, torch.float64, None, flips or None)
    return y, g, dx, rep


def flip_impacts(case, band=BAND, limit=8):
    """Diagnostic: for up to `limit` at-risk units per tapped tensor, the largest relative change (max-norm over a gradient
    tensor / max|that tensor|) caused by inverting that ONE unit's kink decision. -> [(tap, index, |z64|/eps, impact, where)]"""
    sv = survey(case, band)
    _, g0, dx0, _ = run(case, torch.float64)
    out = []
    for name, s in sv.items():
        for idx in s["at_risk"].nonzero()[:limit]:
            f = torch.zeros_like(s["at_risk"])
            f[tuple(idx)] = True
            _, g, dx, _ = run(case, torch.float64, None, {name: f})
            worst, where = float((dx - dx0).abs().max() / dx0.abs().max()), "dx"
            for k in g0:
                v = float((g[k] - g0[k]).abs().max() / (g0[k].abs().max() + 1e-300))
                if v > worst:
                    worst, where = v, k
            out.append((name, tuple(idx.tolist()), float(s["z64"].abs()[tuple(idx)]) / max(s["eps"], 1e-300), worst, where))
    return out


def saved_from_tap(case, name, z, keep=None):
    """The tensor gi_net_saved_activation holds behind tap `name`, from the tap z: the encoder and the critic keep
    LeakyReLU(0.2)(z) (the innermost level relu(z): its only consumer is the uprelu), the decoder relu(z) after dropout."""
    if name.startswith("u") or (case["kind"] == "unet" and name == f"d{case['nd']}"):
        a = torch.relu(z)
        return a * keep.to(a.dtype) * 2.0 if keep is not None else a
    return torch.where(z > 0, z, 0.2 * z)


def _rel_max(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))


def _rel_l2(a, b):
    return float((a.double() - b).norm() / (b.norm() + 1e-300))


def _errors(case, impl, ref, skip=()):
    """Per compared tensor the error of `impl` (dict y, stats, acts, grads, dx; entries may be missing) against
    ref = (y64, grads64, dx64) and the fp64 forward, in the norm of its class: {(class, name): error}. Output, running
    statistics: max-norm relative to max|ref|; saved activations: max-norm in units of the pre-activation (dropout's factor 2
    removed), ABSOLUTE, to be held against eps16; gradients: relative L2."""
    y64, g64, dx64 = ref
    f64 = forward64(case)
    out = {}
    if impl.get("y") is not None:
        out[("out", "y")] = _rel_max(impl["y"], y64)
    for k, v in (impl.get("stats") or {}).items():
        out[("stat", k)] = _rel_max(v, f64["stats"][k])
    for name, a in (impl.get("acts") or {}).items():
        keep = f64["taps"].get(name + ".keep")
        want = saved_from_tap(case, name, f64["taps"][name], keep)
        out[("tap", name)] = float((a.double() - want).abs().max()) / (2.0 if keep is not None else 1.0)
    for name, g in (impl.get("grads") or {}).items():
        if name not in skip:
            out[("grad", name)] = _rel_l2(g, g64[name])
    if impl.get("dx") is not None:
        out[("grad", "dx")] = _rel_l2(impl["dx"], dx64)
    return out


def yardstick(case):
    """What fp16 storage has to cost on this case (cached): dict(err = {(class, name): error of the storage-rounded restatement
    in _errors' norms} - the saved activations' entries are eps16 of their tap -, eps16, rep = kink_reference's report with
    the restatement standing where an implementation stands). The restatement's gradients are compared with the fp64 oracle
    evaluated with the restatement's own kink decisions inside the band."""
    def go():
        r = restated(case)
        dec = {k: v > 0 for k, v in r["taps"].items() if not k.endswith(".keep")}
        y, g, dx, rep = kink_reference(case, dec, fp16=True)
        err = _errors(case, {"y": r["y"], "stats": r["stats"], "grads": r["grads"], "dx": r["dx"]}, (y, g, dx))
        e16 = eps16(case)
        for name in e16:
            err[("tap", name)] = e16[name]
        return {"err": err, "eps16": e16, "rep": rep}
    return _cached(case, "yardstick", go)


def fp16_parity(case, impl, ref, rep, skip=()):
    """The fp16 bound: every tensor of `impl` may err at most K times what the restatement errs (`yardstick`) plus FLOOR32 (of
    max|z64| for a saved activation, whose error is absolute), and the band the
    reference was evaluated with (`rep`, from kink_reference(case, impl's decisions, fp16=True), ref = its y, grads, dx) holds
    at most BAND_SHARE_CAP of the live units, of which at most FLIP_SHARE_CAP were decided by impl.
    -> (records, failures): records = [dict(cls, name, err, yardstick, ratio)], failures = [message]."""
    yd = yardstick(case)
    errs = _errors(case, impl, ref, skip)
    records, bad = [], []
    for (cls, name), e in errs.items():
        y = yd["err"][(cls, name)]
        # A ONE-element gradient (the generator's u1 bias, the critic's Linear bias) has no norm to average over: its error is one
        # draw of a zero-mean sum, and so is the restatement's - the ratio of two such draws exceeds 4 one time in six whatever the
        # implementation does (measured on MI355X: 0.28 ... 7.4 over eleven cases, median 1.1). Its yardstick is therefore a SCALE:
        # at least the restatement's relative L2 error on the weight gradient of the same layer, whose every element is the same
        # sum over the same output-gradient tensor, weighted by an activation instead of by one.
        sibling = name[:-len("bias")] + "weight"
        if cls == "grad" and name.endswith(".bias") and case["P"][name].size == 1 and ("grad", sibling) in yd["err"]:
            y = max(y, yd["err"][("grad", sibling)])
        floor = FLOOR32 * (float(forward64(case)["taps"][name].abs().max()) if cls == "tap" else 1.0)
        ratio = e / (y + floor / K)          # <= K exactly when the tensor passes
        records.append({"cls": cls, "name": name, "err": e, "yardstick": y, "ratio": ratio})
        if not e <= K * y + floor:
            bad.append(f"{cls} {name}: error {e:.3e} > {K:g} x yardstick {y:.3e} + {floor:.1e} (ratio {ratio:.2f})")
    units = max(rep["units"], 1)
    if rep["at_risk"] / units > BAND_SHARE_CAP:
        bad.append(f"{rep['at_risk']} of {rep['units']} live units lie inside the fp16 band ({rep['at_risk'] / units:.2%} > {BAND_SHARE_CAP:.0%})")
    if rep["flipped"] / units > FLIP_SHARE_CAP:
        bad.append(f"{rep['flipped']} of {rep['units']} kink decisions taken from the implementation ({rep['flipped'] / units:.2e} > {FLIP_SHARE_CAP:.0e})")
    if rep["outside"]:
        bad.append(f"{rep['outside']} kink decisions differ outside the band (worst {rep['outside_worst']:.2f} band widths)")
    return records, bad


def worst_by_class(records):
    """{class: record with the largest ratio}"""
    out = {}
    for r in records:
        if r["cls"] not in out or r["ratio"] > out[r["cls"]]["ratio"]:
            out[r["cls"]] = r
    return out
