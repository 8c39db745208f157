"""Drop-in for the reference's lib/fid/inception.py: the FID variant of Inception-V3 up to its 2048-wide pool3 features, on
`gi_inception_*` (csrc/inception.hip: one MFMA implicit-GEMM template for the 94 convolutions, BatchNorm folded at
sync_weights, forward only).

The reference downloads the published weight file when the model is built. This class NEVER fetches anything: parameters
start at zero and `load_state_dict` takes the published file's keys (`Conv2d_1a_3x3.conv.weight`, `...bn.weight|bias|
running_mean|running_var`, `Mixed_5b.branch1x1...`), e.g. `model.load_state_dict(torch.load(local_path))`."""
import ctypes as C

import torch
import torch.nn as nn

from ... import backend as B


def _inventory():
    """[(key, shape, float offset)] and the parameter count, from a context-free handle (works without a GPU)."""
    lib = B.lib()
    hd = C.c_void_p()
    B.check(lib.gi_inception_create(None, B.GI_F32, 1, C.byref(hd)))
    try:
        out = []
        name = C.create_string_buffer(128)
        shape = (C.c_int * 4)()
        off = C.c_int64()
        for i in range(lib.gi_inception_num_tensors(hd)):
            B.check(lib.gi_inception_tensor_desc(hd, i, C.cast(name, C.c_void_p), 128, C.cast(shape, C.c_void_p),
                                                 C.cast(C.pointer(off), C.c_void_p)))
            out.append((name.value.decode(), tuple(int(s) for s in shape if s > 0), int(off.value)))
        return out, int(lib.gi_inception_param_floats(hd))
    finally:
        lib.gi_inception_destroy(hd)


class InceptionV3(nn.Module):
    """Inception-V3 feature extractor for FID (reference lib/fid/inception.py:16-160), output block 3 only."""

    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks=[DEFAULT_BLOCK_INDEX], resize_input=True, normalize_input=True, requires_grad=False,
                 use_fid_inception=True, dtype="fp16", max_batch=50):
        super().__init__()
        if sorted(output_blocks) != [3]:
            raise NotImplementedError("InceptionV3: only output block 3 (the 2048-wide pool3 features, the one FID uses) is built; "
                                      "got output_blocks=%r" % (list(output_blocks),))
        if not resize_input:
            raise NotImplementedError("InceptionV3: resize_input=False is not supported: the input kernel always resizes to 299x299")
        if not normalize_input:
            raise NotImplementedError("InceptionV3: normalize_input=False is not supported: the input kernel always maps [0,1] to [-1,1]")
        if requires_grad:
            raise NotImplementedError("InceptionV3: requires_grad=True is not supported: the HIP network is forward only")
        if not use_fid_inception:
            raise NotImplementedError("InceptionV3: use_fid_inception=False (torchvision's own variant and weights) is not supported")
        self.output_blocks = [3]
        self.last_needed_block = 3
        self.resize_input, self.normalize_input = True, True
        self.compute_dtype = B.dtype_code(dtype)
        self.max_batch = int(max_batch)
        self._inventory, count = _inventory()
        self.register_buffer("flat", torch.zeros(count))
        self._handles = {}
        self._dirty = True
        self._debug = None
        self._program = None

    # ---- state_dict in the published file's naming -------------------------------------------------------------------------
    def _views(self):
        out = {}
        for key, shape, off in self._inventory:
            n = 1
            for s in shape:
                n *= s
            out[key] = self.flat[off: off + n].view(*shape)
        return out

    def state_dict(self, *args, **kw):
        return {k: v.detach().clone() for k, v in self._views().items()}

    def load_state_dict(self, sd, strict=True):
        """Copies the published file's tensors; `fc.*` and `*.num_batches_tracked` are ignored. Returns the missing keys
        (strict: raises if there are any)."""
        views = self._views()
        seen = set()
        for k, v in sd.items():
            if k.startswith("fc.") or k.endswith("num_batches_tracked"):
                continue
            if k in views:
                v = torch.as_tensor(v)
                if tuple(v.shape) != tuple(views[k].shape):
                    raise RuntimeError("InceptionV3.load_state_dict: %s has shape %s, expected %s" % (k, tuple(v.shape), tuple(views[k].shape)))
                views[k].copy_(v.to(views[k].device, torch.float32))
                seen.add(k)
        missing = [k for k in views if k not in seen]
        if strict and missing:
            raise RuntimeError("InceptionV3.load_state_dict: missing keys %s" % missing)
        self._dirty = True
        return missing

    def _handle(self, dev):
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        if key not in self._handles:
            lib, ctx = B.lib(), B.get_ctx(dev)
            hd = C.c_void_p()
            B.check(lib.gi_inception_create(ctx, self.compute_dtype, self.max_batch, C.byref(hd)))
            if lib.gi_inception_param_floats(hd) != self.flat.numel():
                raise B.BackendError("InceptionV3: parameter layout mismatch")
            ws = torch.empty(lib.gi_inception_workspace_bytes(hd) + 256, dtype=torch.uint8, device=dev)
            off = (-ws.data_ptr()) % 256
            B.check(lib.gi_inception_bind(hd, B.ptr(self.flat), ws.data_ptr() + off, ws.numel() - off))
            self._handles[key] = (hd, ws)
            self._dirty = True
        hd = self._handles[key][0]
        if self._dirty:
            for h2, _ in self._handles.values():
                B.check(B.lib().gi_inception_sync_weights(h2))
            self._dirty = False
        return hd

    def _check(self, x):
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] not in (1, 3):
            raise B.BackendError("InceptionV3 takes (n,1|3,H,W) float32 tensors in [0,1] on the gfx950 device")
        if self.flat.device != x.device:
            raise B.BackendError("InceptionV3 parameters live on %s, input on %s: call .to(device)" % (self.flat.device, x.device))

    @torch.no_grad()
    def features(self, x):
        """(n, 2048) float32 pool3 features; batches larger than max_batch run in slices (a picture's features do not depend
        on the batch it arrives in)."""
        self._check(x)
        x = x.detach().contiguous()
        hd = self._handle(x.device)
        n, c, h, w = x.shape
        out = torch.empty(n, 2048, dtype=torch.float32, device=x.device)
        for i in range(0, n, self.max_batch):
            k = min(self.max_batch, n - i)
            B.check(B.lib().gi_inception_features(hd, B.ptr(x[i:i + k]), k, c, h, w, B.ptr(out[i:i + k])))
        return out

    def forward(self, inp):
        """[features (n, 2048, 1, 1)], as the reference returns for output_blocks=[3]."""
        return [self.features(inp).view(-1, 2048, 1, 1)]

    def debug_forward_convs(self, x, nconvs):
        """Runs the first nconvs convolutions only (tests: which kernel served a shape, backend.last_kernel())."""
        self._check(x)
        x = x.detach().contiguous()
        hd = self._handle(x.device)
        B.check(B.lib().gi_inception_debug_forward_convs(hd, B.ptr(x), x.shape[0], x.shape[1], x.shape[2], x.shape[3], int(nconvs)))

    STEP_KINDS = ("conv", "max_s2", "avg_s1", "max_s1")

    @staticmethod
    def program():
        """The forward program, step by step, from a context-free handle (works without a GPU): a list of dicts with kind
        (STEP_KINDS), conv (index into the 94 convolutions or -1), cin / cout views (C, H, W), src (-1: the resized input),
        dst, ldout and coffout."""
        lib = B.lib()
        hd = C.c_void_p()
        B.check(lib.gi_inception_create(None, B.GI_F32, 1, C.byref(hd)))
        try:
            out = []
            kind, conv = C.c_int(), C.c_int()
            i3, o3, r4 = (C.c_int * 3)(), (C.c_int * 3)(), (C.c_int * 4)()
            for i in range(lib.gi_inception_num_steps(hd)):
                B.check(lib.gi_inception_step_desc(hd, i, C.cast(C.pointer(kind), C.c_void_p), C.cast(C.pointer(conv), C.c_void_p),
                                                   C.cast(i3, C.c_void_p), C.cast(o3, C.c_void_p), C.cast(r4, C.c_void_p)))
                out.append(dict(kind=InceptionV3.STEP_KINDS[kind.value], conv=int(conv.value), in_chw=tuple(int(a) for a in i3),
                                out_chw=tuple(int(a) for a in o3), src=int(r4[0]), dst=int(r4[1]), ldout=int(r4[2]), coffout=int(r4[3])))
            return out
        finally:
            lib.gi_inception_destroy(hd)

    def debug_forward_steps(self, x, nsteps):
        """Runs the input kernel and the first nsteps steps of the program (tests: debug_read of step nsteps - 1)."""
        self._check(x)
        x = x.detach().contiguous()
        hd = self._handle(x.device)
        B.check(B.lib().gi_inception_debug_forward_steps(hd, B.ptr(x), x.shape[0], x.shape[1], x.shape[2], x.shape[3], int(nsteps)))
        self._debug = (x.device, x.shape[0])

    def debug_read(self, step, which):
        """fp32 NCHW copy of step's input view (which = 0), output view (1) or whole destination rows (2); only directly after
        debug_forward_steps(x, step + 1), for that x's batch size."""
        if self._debug is None:
            raise B.BackendError("InceptionV3.debug_read: call debug_forward_steps first")
        dev, n = self._debug
        hd = self._handle(dev)
        d = self.program_cached()[step]
        c, h, w = d["in_chw"] if which == 0 else d["out_chw"]
        if which == 2:
            c = d["ldout"]
        out = torch.empty(n, c, h, w, dtype=torch.float32, device=dev)
        B.check(B.lib().gi_inception_debug_read(hd, int(step), int(which), n, B.ptr(out)))
        return out

    def program_cached(self):
        if self._program is None:
            self._program = self.program()
        return self._program

    def __del__(self):
        try:
            for hd, _ in self._handles.values():
                B.lib().gi_inception_destroy(hd)
        except Exception:
            pass
