#!/usr/bin/env python3
"""Which implicit-GEMM kernel serves which layer, as a table: one row per (shape, fused epilogue, option set).

  --launch   drives gi_conv_s2_forward_ex / gi_convT_s2_forward_ex on the GPU and records, per row, gi_debug_last_kernel, the
             returned fields of gi_igemm_ex and a sha256 of the output tensor (same kernel, same arguments, same grid => same bits)
  --plan     the same rows without the hash through gi_debug_igemm_plan: host arithmetic only, no GPU

GI_LIB_PATH names the library as for the other A/B tools; --commit is written into the header. The case list is generated:
the shapes of tests/test_dispatch_gpu.py (CONV_FWD, CONVT_FWD, DGRAD) and tests/test_options_gpu.py (LAYER_OPTIONS), each with
every epilogue and, separately, under every option set; neighbours of the tile-count thresholds; map widths that are and are not
powers of two; non-square maps; channel counts that the LDS-DMA kernels do not take; workspace absent / too small; fp32.
--launch keeps every tensor within 64 MiB: a shape whose tensors are larger runs with its batch halved until they fit (the
critic's conv2 at n = 64 becomes n = 32, where it has 1024 workgroups: still beyond every threshold). Workspace sizes between
"too small for any split" and "one buffer per split" are left out: there the generic kernel adds its splits with fp32 atomics
and the output bits depend on the arrival order.

usage: python tools/dispatch_table.py --launch|--plan [--commit ID] [--out FILE]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)

F32, F16 = 0, 1
EPILOGUES = ["none", "stat", "mask", "mask+bits", "bwd", "bwd-upper"]
OPTION_SETS = [{}, {"GI_IGEMM8": 0}, {"GI_IGEMM8": 2}, {"GI_IGEMM6": 0}, {"GI_IGEMM5": 0}, {"GI_IGEMM5": 1}, {"GI_IGEMM5": 2},
               {"GI_IGEMM7": 0}, {"GI_IGEMM7": 0, "GI_IGEMM_FIXUP": 0}, {"GI_IGEMM_VARIANT": 1}, {"GI_IGEMM7_WAVES": 4}]
WS_FULL = 64 << 20     # bytes; what the single-layer tests pass
LIMIT = 64 << 20       # largest tensor of a --launch row
FIELDS = ["rc", "error", "kernel", "ntiles_out", "mask_applied", "bwd_applied", "stat_used"]


class PlanInfo(C.Structure):
    """gi_igemm_plan_info (include/ganinpaint.h)"""
    _fields_ = [("name", C.c_char * 48), ("grid", C.c_int), ("splitk", C.c_int), ("ntiles_out", C.c_int),
                ("mask_applied", C.c_int), ("bwd_applied", C.c_int), ("stat_used", C.c_int), ("c1w_applied", C.c_int),
                ("c1w_blocks", C.c_int), ("pool_applied", C.c_int), ("fold_applied", C.c_int)]


OFFER_FOLD, OFFER_C1W, OFFER_POOL2, OFFER_BIAS = 1, 2, 4, 8


CASE_FIELDS = ["dtype", "mode", "n", "Hs", "Ws", "cin", "cout", "relu_in", "relu_cend", "epi", "opts", "ws_bytes"]


def dumps(doc):
    """a table as text: a header, then one line per row (the case's fields, then the recorded ones), sorted by case"""
    fields = FIELDS + (["sha256"] if doc["how"] == "launch" else [])
    rows = sorted(doc["rows"], key=lambda r: json.dumps(r["case"], sort_keys=True))
    head = {"commit": doc["commit"], "how": doc["how"], "case_fields": CASE_FIELDS, "fields": fields}
    lines = [json.dumps([r["case"][f] for f in CASE_FIELDS] + [r[f] for f in fields], sort_keys=True) for r in rows]
    return json.dumps(head)[:-1] + ', "rows": [\n' + ",\n".join(lines) + "\n]}\n"


def loads(text):
    doc = json.loads(text)
    nc = len(doc["case_fields"])
    doc["rows"] = [{"case": dict(zip(doc["case_fields"], r[:nc])), **dict(zip(doc["fields"], r[nc:]))} for r in doc["rows"]]
    return doc


def _test_shapes():
    """(mode, n, Hs, Ws, cin, cout, relu_in, relu_cend) of the tests' tables; mode 0: Conv2d 4x4/s2 (Hs = H / 2), 1: sub-pixel phases"""
    conv_fwd = [(32, 128, 64, 128), (32, 64, 128, 256), (32, 32, 256, 512), (32, 16, 512, 512), (32, 8, 512, 512), (32, 4, 512, 512),
                (64, 128, 64, 128), (64, 64, 128, 256), (64, 32, 256, 512)]
    convt_fwd = [(32, 2, 512, 512, 0), (32, 4, 1024, 512, 512), (32, 8, 1024, 512, 512), (32, 16, 1024, 256, 512), (32, 32, 512, 128, 256),
                 (32, 64, 256, 64, 128)]
    dgrad = [(0, 32, 128, 64, 256), (0, 32, 64, 128, 512), (0, 32, 32, 256, 1024), (1, 32, 32, 256, 128), (1, 32, 16, 512, 256),
             (1, 32, 64, 128, 64), (1, 64, 64, 128, 64), (1, 64, 16, 512, 256), (1, 64, 32, 256, 128)]
    layer_options = [(0, 16, 128, 64, 128), (1, 8, 32, 256, 128), (1, 8, 32, 128, 64), (1, 16, 32, 256, 128), (0, 32, 16, 512, 512),
                     (1, 32, 4, 1024, 512), (1, 4, 8, 512, 256), (0, 32, 128, 64, 128), (1, 32, 32, 256, 128), (1, 32, 64, 128, 64)]
    out = [(0, n, hw // 2, hw // 2, cb, ca, 0, 0) for n, hw, cb, ca in conv_fwd]
    out += [(1, n, hw, hw, ca, cb, 1 if cend else 0, cend) for n, hw, ca, cb, cend in convt_fwd]
    out += [(m, n, hw // 2 if m == 0 else hw, hw // 2 if m == 0 else hw, ci, co, 0, 0) for m, n, hw, ci, co in dgrad + layer_options]
    return out


def _case(mode, n, Hs, Ws, cin, cout, relu_in=0, relu_cend=0, epi="none", opts=None, ws=WS_FULL, dtype=F16):
    return {"dtype": dtype, "mode": mode, "n": n, "Hs": Hs, "Ws": Ws, "cin": cin, "cout": cout, "relu_in": relu_in, "relu_cend": relu_cend,
            "epi": epi, "opts": dict(opts or {}), "ws_bytes": ws}


def tensor_bytes(c):
    es = 2 if c["dtype"] == F16 else 4
    px = c["n"] * c["Hs"] * c["Ws"]
    return max(px * (4 if c["mode"] == 0 else 1) * c["cin"] * es, px * (4 if c["mode"] == 1 else 1) * c["cout"] * es)


def cases():
    rows, seen = [], set()

    def add(c):
        while tensor_bytes(c) > LIMIT and c["n"] > 1:
            c["n"] //= 2
        key = json.dumps(c, sort_keys=True)
        if key not in seen:
            seen.add(key)
            rows.append(c)

    shapes = _test_shapes()
    for s in shapes:
        for epi in EPILOGUES:
            add(_case(*s, epi=epi))
        for o in OPTION_SETS[1:]:
            add(_case(*s, opts=o))
    # threshold neighbours: 16x16 small grids hold one 256-pixel tile per image
    for n in (127, 128, 255, 256, 511, 512):            # halo kernels, gather: tiles = workgroups = n
        add(_case(0, n, 16, 16, 64, 128))
    for n in (31, 32, 63, 64, 127, 128):                # sub-pixel phases: 4 n
        add(_case(1, n, 16, 16, 64, 128))
        add(_case(1, n, 16, 16, 128, 64))                # dual-px tiles: 2 n workgroups
    for n in (127, 128, 255, 256):                      # igemm3 (halo kernels off): 128..255 tiles -> 64-wide N tiles
        add(_case(0, n, 16, 16, 64, 128, opts={"GI_IGEMM5": 0}))
    for n in (29, 30, 31, 32, 33):                      # igemm7: 63 / 64 tiles of 128 x 128 switch the N tile
        add(_case(0, n, 8, 8, 512, 512))
    for n in (7, 8):
        add(_case(1, n, 8, 8, 512, 512))
    # map widths (24 is no power of two), non-square maps (Hs % TH != 0 and == 0), both modes, with and without the input ReLU
    for Ws in (4, 8, 16, 24, 32, 64):
        for Hs in (Ws, 12 if Ws != 12 else 20, 2 * Ws):
            for mode in (0, 1):
                for relu in (0, 1):
                    add(_case(mode, 16, Hs, Ws, 128, 128, relu_in=relu))
    for cin in (32, 64, 96):
        for cout in (64, 128, 192):
            for mode in (0, 1):
                add(_case(mode, 16, 16, 16, cin, cout))
                add(_case(mode, 4, 16, 16, cin, cout, dtype=F32))
    # workspace absent (the entries then pass no tickets either) / too small for any split
    for s in [(0, 32, 8, 8, 512, 512), (1, 32, 4, 4, 1024, 512), (0, 32, 2, 2, 512, 512), (1, 4, 8, 8, 512, 256), (0, 16, 64, 64, 64, 128)]:
        for ws in (0, 4096):
            for o in ({}, {"GI_IGEMM7": 0}, {"GI_IGEMM7": 0, "GI_IGEMM_FIXUP": 0}):
                add(_case(*s, opts=o, ws=ws))
    for s in [(0, 8, 16, 16, 64, 128), (1, 8, 16, 16, 128, 64), (0, 32, 4, 4, 256, 256), (1, 32, 4, 4, 256, 256), (0, 64, 32, 32, 32, 64)]:
        for epi in ("none", "stat"):
            add(_case(*s, epi=epi, dtype=F32))
            add(_case(*s, epi=epi, dtype=F32, opts={"GI_IGEMM_FIXUP": 0}))
    return rows


def out_pixels(c):
    return c["n"] * c["Hs"] * c["Ws"] * (4 if c["mode"] == 1 else 1)


def fill_ex(ex, c, p):
    """the epilogue of a case; p(name, bytes) -> a pointer (device memory for --launch, any non-null number for --plan)"""
    cout, px, epi = c["cout"], out_pixels(c), c["epi"]
    ex.relu_cend = c["relu_cend"]
    if epi == "stat":
        ex.stat_acc, ex.stat_reps, ex.stat_pg = p("acc", 0), 2, 0
    if epi.startswith("mask"):
        ex.mask, ex.ldmask, ex.mask_slope = p("mask", px * cout * 2), cout, 0.2
        if epi == "mask+bits":
            ex.mask_bits = p("bits", px * 8)
    if epi.startswith("bwd"):
        cb = cout // 2 if epi == "bwd-upper" else cout
        base = p("vec", 16 * cout)
        ex.bwd_x, ex.bwd_ldx = p("bwd_x", px * cb * 2), cb
        ex.bwd_scale, ex.bwd_shift, ex.bwd_mean, ex.bwd_inv, ex.bwd_stride = base, base + 4 * cb, base + 8 * cb, base + 12 * cb, 4 * cb
        ex.bwd_slope, ex.bwd_acc, ex.bwd_reps, ex.bwd_pg = 0.2, p("acc", 0), 2, 0
        if epi == "bwd-upper":
            ex.bwd_c0, ex.bwd_c = cb, cb


def with_options(B, opts, fn):
    for k, v in opts.items():
        B.set_option(k, v)
    try:
        return fn()
    finally:
        for k in opts:
            B.set_option(k, -1)


def plan_row(B, c, offered=0, ex_hook=None):
    """one row through gi_debug_igemm_plan (no GPU); ex_hook(ex) may add to the epilogue"""
    ex = B.IgemmEx()
    fill_ex(ex, c, lambda name, nbytes: 1 << 20)
    if ex_hook:
        ex_hook(ex)
    info = PlanInfo()

    def call():
        return B.lib().gi_debug_igemm_plan(c["dtype"], c["mode"], c["n"], c["Hs"], c["Ws"], c["cin"], c["cin"], c["cout"], c["cout"], c["relu_in"], 0,
                                           c["ws_bytes"], 1 if c["ws_bytes"] > 0 else 0, C.byref(ex), offered, C.byref(info))
    rc = with_options(B, c["opts"], call)
    row = {"rc": rc, "error": B.lib().gi_last_error().decode() if rc else "", "kernel": info.name.decode() if rc == 0 else ""}
    for f in ("ntiles_out", "mask_applied", "bwd_applied", "stat_used"):
        row[f] = getattr(info, f) if rc == 0 else 0
    row["_info"] = info
    return row


class Launcher:
    def __init__(self, B):
        import torch
        self.B, self.torch, self.key, self.t = B, torch, None, {}
        self.ws = torch.zeros(WS_FULL // 4, dtype=torch.float32, device="cuda")
        self.lib, self.ctx = B.lib(), B.get_ctx()

    def operands(self, c):
        torch, key = self.torch, (c["dtype"], c["mode"], c["n"], c["Hs"], c["Ws"], c["cin"], c["cout"])
        if key != self.key:
            self.t, self.key = {}, key
            torch.cuda.empty_cache()
            dt = torch.float16 if c["dtype"] == F16 else torch.float32
            g = torch.Generator(device="cuda").manual_seed(1234)
            k = 4 if c["mode"] == 0 else 1
            self.t["x"] = (torch.rand((c["n"] * c["Hs"] * c["Ws"] * k, c["cin"]), device="cuda", generator=g) - 0.3).to(dt)
            ca, cb = (c["cout"], c["cin"]) if c["mode"] == 0 else (c["cin"], c["cout"])
            w = (torch.rand((ca, 4, 4, cb), device="cuda", generator=g) * 2 - 1) * 0.02
            self.t["w"] = torch.empty(ca * 16 * cb, dtype=dt, device="cuda")
            wp = self.B.ptr(self.t["w"])
            self.B.check(self.lib.gi_pack_weights(self.ctx, c["dtype"], self.B.ptr(w), ca, cb, wp if c["mode"] == 0 else None, None if c["mode"] == 0 else wp))
            self.t["out"] = torch.empty((out_pixels(c), c["cout"]), dtype=dt, device="cuda")
            self.g = g
        return self.t

    def aux(self, name, nbytes, c):
        torch, t = self.torch, self.t
        if name == "acc":
            t["acc"] = torch.zeros(self.lib.gi_stat_acc_words(c["cout"]), dtype=torch.int64, device="cuda")
        elif name not in t or t[name].numel() * t[name].element_size() != nbytes:
            if name == "vec":
                t[name] = torch.rand(nbytes // 4, device="cuda", generator=self.g) + 0.5
            elif name == "bits":
                t[name] = torch.randint(0, 256, (nbytes,), device="cuda", generator=self.g, dtype=torch.uint8)
            else:
                t[name] = (torch.rand(nbytes // 2, device="cuda", generator=self.g) - 0.5).half()
        return t[name].data_ptr()

    def row(self, c):
        B, t = self.B, self.operands(c)
        ex = B.IgemmEx()
        fill_ex(ex, c, lambda name, nbytes: self.aux(name, nbytes, c))
        t["out"].view(self.torch.int16).fill_(0x7e7e)
        self.ws.fill_(float("nan"))
        fn = self.lib.gi_conv_s2_forward_ex if c["mode"] == 0 else self.lib.gi_convT_s2_forward_ex
        k = 2 if c["mode"] == 0 else 1
        ws = self.ws if c["ws_bytes"] > 0 else None

        def call():
            rc = fn(self.ctx, c["dtype"], B.ptr(t["x"]), B.ptr(t["w"]), B.ptr(t["out"]), c["n"], k * c["Hs"], k * c["Ws"], c["cin"], c["cin"],
                    c["cout"], c["cout"], c["relu_in"], 0, B.ptr(ws), c["ws_bytes"], C.byref(ex))
            self.torch.cuda.synchronize()
            return rc
        rc = with_options(B, c["opts"], call)
        row = {"rc": rc, "error": self.lib.gi_last_error().decode() if rc else "", "kernel": B.last_kernel() if rc == 0 else ""}
        for f in ("ntiles_out", "mask_applied", "bwd_applied", "stat_used"):
            row[f] = getattr(ex, f) if rc == 0 else 0
        row["sha256"] = hashlib.sha256(t["out"].view(self.torch.int16).cpu().numpy().tobytes()).hexdigest() if rc == 0 else ""
        return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch", action="store_true")
    ap.add_argument("--plan", action="store_true")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.launch != a.plan, "one of --launch / --plan"
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    cs = sorted(cases(), key=lambda c: (c["dtype"], c["mode"], c["n"], c["Hs"], c["Ws"], c["cin"], c["cout"])) if a.launch else cases()
    rows = []
    run = Launcher(B).row if a.launch else (lambda c: {k: v for k, v in plan_row(B, c).items() if k != "_info"})
    for i, c in enumerate(cs):
        r = run(c)
        rows.append({"case": c, **r})
        print(f"{i:4d} {json.dumps(c, sort_keys=True)} -> {r['kernel'] or r['error']}", flush=True)
    text = dumps({"commit": a.commit, "how": "launch" if a.launch else "plan", "rows": rows})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(f"{len(rows)} rows")


if __name__ == "__main__":
    main()
