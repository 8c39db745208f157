#!/usr/bin/env python3
"""sha256 of everything the network schedules of csrc/net.hip produce, over a fixed list of small cases -> one JSON file.
The networks are bit-reproducible (tests/test_nets_gpu.py, test_*_reproducible), so two builds of the library that are meant to
compute the same thing must give EQUAL records: run once per build in a fresh process (GI_LIB_PATH names the other build) and
compare with --compare. Hashed per case: output, input gradient, flat parameter gradients (after every phase of a phased
backward), running statistics, the dropout masks the library drew, the gradient penalty's value.
usage: net_hashes.py OUT.json [case-name substring]   |   net_hashes.py --compare A.json B.json"""
import hashlib, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np, torch
import gan_inpainting_amd  # noqa
from gan_inpainting_amd import backend as B
from gan_inpainting_amd.lib.models import networks
from oracle import params as op


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def normal(seed, shape):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(size=shape, dtype=np.float32)).cuda()


def load(net, P):
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in P.items()})
    net = net.to("cuda")
    (net.phys if hasattr(net, "phys") else net).set_loss_scale(1.0)
    return net


def stats(net):
    return {"stat:" + k: v.float() for k, v in net.state_dict().items() if "running" in k}


def unet(dtype, nd, N, HW, norm="batch", out_c=1, ngf=64, mode="train", dropout=False, need_dx=True, need_wgrad=True, phases=None, seed=100):
    """mode: train | eval | inference. phases: backward through gi_net_backward_phase in these phases instead of one call."""
    P = op.make_unet_params(seed + nd + HW, num_downs=nd, ngf=ngf, out_c=out_c, norm=norm)
    net = load(networks.UnetGenerator(1, out_c, nd, ngf, networks.get_norm_layer(norm), use_dropout=dropout, dtype=dtype), P)
    net = net.train() if mode == "train" else net.eval()
    g = net.phys if hasattr(net, "phys") else net
    if dropout:
        g.set_dropout_seed(1234)
    ground, mask = op.synth_batch(seed + 7, N, HW, HW)
    x = torch.from_numpy(ground * (1 - mask)).cuda()
    dy = normal(seed, (N, out_c, HW, HW))
    g.zero_grad()
    y, s, gen = g._forward_raw(x, inference=mode == "inference")
    out = {"y": y}
    if dropout and mode == "train":
        out.update({f"mask{k}": v for k, v in g.dropout_masks().items()})
    if phases is None and (need_dx or need_wgrad) and mode != "inference":
        dx = g._backward_raw(s, gen, dy, need_dx, need_wgrad)
        if need_dx:
            out["dx"] = dx
    for ph in phases or ():
        B.check(B.lib().gi_net_backward_phase(g._handle, s, B.ptr(dy), None, 1, ph))
        out[f"grads_after_phase{ph}"] = g.flat_grads().clone()
    torch.cuda.synchronize()
    out["grads"] = g.flat_grads()
    out.update(stats(net))
    return out


def patchgan(dtype, N, HW, groups=2, sigmoid=False, need_dx=True, phases=None, seed=66):
    net = load(networks.PatchGANDiscriminator(sigmoid=sigmoid, image_size=HW, dtype=dtype), op.make_patchgan_params(seed, HW, HW)).train()
    x = torch.from_numpy(op.synth_batch(seed + 2, N, HW, HW)[0]).cuda()
    dy = normal(seed, (N, 1))
    net.zero_grad()
    y, s, gen = net._forward_raw(x, groups)
    out = {"y": y}
    if phases is None:
        dx = net._backward_raw(s, gen, dy, need_dx, True)
        if need_dx:
            out["dx"] = dx
    for ph in phases or ():
        B.check(B.lib().gi_net_backward_phase(net._handle, s, B.ptr(dy), None, 1, ph))
        out[f"grads_after_phase{ph}"] = net.flat_grads().clone()
    torch.cuda.synchronize()
    out["grads"] = net.flat_grads()
    out.update(stats(net))
    return out


def penalty(dtype, N=4, HW=64, seed=77):
    net = load(networks.PatchGANDiscriminator(sigmoid=False, image_size=HW, dtype=dtype), op.make_patchgan_params(seed, HW, HW)).train()
    real = torch.from_numpy(op.synth_batch(seed + 1, N, HW, HW)[0]).cuda()
    fake = torch.from_numpy(op.synth_batch(seed + 2, N, HW, HW)[0]).cuda()
    net.zero_grad()
    value = net.gradient_penalty(real, fake, eps=torch.linspace(0.1, 0.9, N), lam=10.0)
    torch.cuda.synchronize()
    out = {"penalty": value, "grads": net.flat_grads()}
    out.update(stats(net))
    return out


CASES = {}
for dt in ("fp16", "fp32"):
    CASES[f"unet-bn-nd6-n2-64-{dt}"] = lambda dt=dt: unet(dt, 6, 2, 64)
    CASES[f"unet-bn-nd7-n3-128-dropout-{dt}"] = lambda dt=dt: unet(dt, 7, 3, 128, dropout=True)   # folds, fused u2 / head, c1w, mask bits, BN-backward fusion
    CASES[f"unet-bn-nd7-n2-128-eval-{dt}"] = lambda dt=dt: unet(dt, 7, 2, 128, mode="eval", need_dx=False, need_wgrad=False)
    CASES[f"unet-bn-nd7-n2-128-inference-{dt}"] = lambda dt=dt: unet(dt, 7, 2, 128, mode="inference")
    CASES[f"unet-bn-nd7-n2-128-eval-dx-{dt}"] = lambda dt=dt: unet(dt, 7, 2, 128, mode="eval", need_wgrad=False)
    CASES[f"segnet-1-4-7-ngf32-n2-128-{dt}"] = lambda dt=dt: unet(dt, 7, 2, 128, out_c=4, ngf=32, mode="eval", need_wgrad=False)   # fp16: head4; fp32: padded GEMM
    for norm in ("instance", "none"):
        CASES[f"unet-{norm}-nd7-n2-128-dropout-{dt}"] = lambda dt=dt, norm=norm: unet(dt, 7, 2, 128, norm=norm, dropout=True)
    for HW in (64, 128):
        for dx in (True, False):
            CASES[f"patchgan-{HW}-n8-g2-{'dx' if dx else 'nodx'}-{dt}"] = lambda dt=dt, HW=HW, dx=dx: patchgan(dt, 8, HW, need_dx=dx)
    CASES[f"patchgan-128-n3-g1-{dt}"] = lambda dt=dt: patchgan(dt, 3, 128, groups=1)    # unaligned population
    CASES[f"penalty-64-n4-{dt}"] = lambda dt=dt: penalty(dt)
CASES["patchgan-128-n8-g2-sigmoid-fp16"] = lambda: patchgan("fp16", 8, 128, sigmoid=True)
for norm in ("batch", "instance"):
    for phases in ((1, 2), (1, 3, 4)):
        CASES[f"unet-{norm}-nd7-n2-128-phases{''.join(map(str, phases))}-fp16"] = lambda norm=norm, phases=phases: unet("fp16", 7, 2, 128, norm=norm, dropout=True, phases=phases)
CASES["patchgan-128-n8-g2-phases12-fp16"] = lambda: patchgan("fp16", 8, 128, phases=(1, 2))


def with_option(name, fn):
    def run():
        B.set_option(name, 0)
        try:
            return fn()
        finally:
            B.set_option(name, -1)
    return run


for name in ("GI_WGRAD_STREAM", "GI_C1W_FUSE", "GI_MASK_BITS", "GI_BN_BWD_FUSE", "GI_HEAD_FAST"):
    CASES[f"unet-bn-nd7-n3-128-dropout-fp16-{name}=0"] = with_option(name, CASES["unet-bn-nd7-n3-128-dropout-fp16"])
    CASES[f"patchgan-128-n8-g2-dx-fp16-{name}=0"] = with_option(name, CASES["patchgan-128-n8-g2-dx-fp16"])


def compare(a, b):
    A, Bb = json.load(open(a)), json.load(open(b))
    bad = [(c, t) for c in sorted(set(A) | set(Bb)) for t in sorted(set(A.get(c, {})) | set(Bb.get(c, {}))) if A.get(c, {}).get(t) != Bb.get(c, {}).get(t)]
    for c, t in bad:
        print(f"DIFFERENT: {c} / {t}")
    print(f"{len(A)} vs {len(Bb)} cases, {sum(len(v) for v in A.values())} tensors, {len(bad)} different")
    return 1 if bad or not A else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    only = sys.argv[2] if len(sys.argv) > 2 else ""
    rec = {}
    for name, fn in CASES.items():
        if only in name:
            rec[name] = {k: sha(v) for k, v in fn().items()}
            print(name, len(rec[name]), "tensors", flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("library", B.LIB_PATH, "->", sys.argv[1])
