"""LPIPS (Zhang et al. 2018, the `lpips` package v0.1 with net='vgg') on the HIP backend: `gi_lpips_*` (csrc/lpips.hip).

    m = LPIPS().to(device); m.load_state_dict(torch.load("vgg16.pth") | torch.load("lpips_vgg.pth"))
    d = m.distance(a, b)          # (n,) device tensor = lpips.LPIPS(net='vgg')(a3, b3, normalize=True) of the grey images repeated over 3 channels

    m = LPIPS(grad=True)...;  d, g = m.distance_and_grad(a, b)   # also g[i] = d d[i] / d a[i] (b constant), (n,1,H,W) float32

The metric of the evaluation pass (lib/models/evaluate.py: calculate_metric(..., lpips_model=m)) and, with grad=True, a training term
(lib/models/loss.py: lpips_loss; csrc/lpips.hip's backward). grad=True binds a second workspace that keeps the feature maps;
without it nothing more is allocated or launched than before. Grey (n,1,H,W) float32
images in [0,1] with H, W multiples of 16; colour inputs are a separate piece of work. No weight file is ever downloaded: the constructor
initialises like torchvision does for `pretrained=False` (He-normal fan_out, zero bias) with lin = 1/C and the published scaling constants,
and only such stand-in weights have been run here."""
import ctypes as C
import re

import torch
import torch.nn as nn

from .. import backend as B


class LPIPS(nn.Module):
    CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)                       # torchvision vgg16.features
    CHANNELS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
    TAP_CHANNELS = (64, 128, 256, 512, 512)                                             # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
    SHIFT = (-.030, -.088, -.188)
    SCALE = (.458, .448, .450)

    def __init__(self, max_pairs=16, grad=False):
        super().__init__()
        self.max_pairs = int(max_pairs)
        self.grad = bool(grad)
        sizes, cin = [], 3
        for cout in self.CHANNELS:
            sizes.append((cout, cin))
            cin = cout
        self._shapes = sizes
        flat = []
        for cout, ci in sizes:
            w = torch.empty(cout, ci, 3, 3)
            nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")
            flat += [w.reshape(-1), torch.zeros(cout)]
        flat += [torch.full((c,), 1.0 / c) for c in self.TAP_CHANNELS]
        flat += [torch.tensor(self.SHIFT), torch.tensor(self.SCALE)]
        self.register_buffer("flat", torch.cat(flat).float())
        self._handles = {}
        self._dirty = True

    # ---- state_dict in the naming of the full LPIPS module over torchvision's feature indices -------------------------------
    def _views(self):
        off, out = 0, {}

        def take(name, shape):
            nonlocal off
            n = 1
            for s in shape:
                n *= s
            out[name] = self.flat[off: off + n].view(*shape)
            off += n
        for i, (cout, ci) in zip(self.CONV_IDX, self._shapes):
            take(f"features.{i}.weight", (cout, ci, 3, 3))
            take(f"features.{i}.bias", (cout,))
        for k, c in enumerate(self.TAP_CHANNELS):
            take(f"lin{k}.model.1.weight", (1, c, 1, 1))
        take("scaling_layer.shift", (1, 3, 1, 1))
        take("scaling_layer.scale", (1, 3, 1, 1))
        assert off == self.flat.numel()
        return out

    def state_dict(self, *args, **kw):
        return {k: v.detach().clone() for k, v in self._views().items()}

    _SLICE = re.compile(r"^net\.slice\d+\.(\d+)\.(weight|bias)$")
    _LINS = re.compile(r"^lins\.(\d+)\.(model\.1\.weight)$")

    @classmethod
    def _canonical(cls, key):
        """`net.slice<k>.<i>.*` (the package's vgg16 wrapper keeps torchvision's indices) -> `features.<i>.*`; `lins.<k>.*` -> `lin<k>.*`."""
        m = cls._SLICE.match(key)
        if m:
            return f"features.{m.group(1)}.{m.group(2)}"
        m = cls._LINS.match(key)
        if m:
            return f"lin{m.group(1)}.{m.group(2)}"
        return key

    def load_state_dict(self, sd, strict=True):
        """A torchvision vgg16 state dict (`features.<i>.weight|bias`) merged with the package's `vgg.pth` (`lin<k>.model.1.weight`), or one
        full LPIPS state dict (`net.slice<k>.<i>.weight|bias`, `lin<k>.model.1.weight`, `scaling_layer.shift|scale`). The classifier and
        unknown keys are ignored; the scaling constants keep their published values when the dict has none. strict: a missing
        convolution or lin tensor raises."""
        views = self._views()
        seen = set()
        for k, v in sd.items():
            k = self._canonical(k)
            if k in views:
                v = torch.as_tensor(v).to(views[k].device, torch.float32)
                if v.numel() != views[k].numel():
                    raise RuntimeError(f"LPIPS.load_state_dict: {k} has shape {tuple(v.shape)}, expected {tuple(views[k].shape)}")
                views[k].copy_(v.reshape(views[k].shape))
                seen.add(k)
        missing = [k for k in views if k not in seen and not k.startswith("scaling_layer.")]
        if strict and missing:
            raise RuntimeError("LPIPS.load_state_dict: missing keys %s" % missing)
        self._dirty = True
        return missing

    def _handle(self, h, w, dev):
        key = (h, w, dev.index, torch.cuda.current_stream(dev).cuda_stream)
        if key not in self._handles:
            lib, ctx = B.lib(), B.get_ctx(dev)
            hd = C.c_void_p()
            B.check(lib.gi_lpips_create(ctx, h, w, self.max_pairs, C.byref(hd)))
            if lib.gi_lpips_param_floats(hd) != self.flat.numel():
                raise B.BackendError("LPIPS: parameter layout mismatch")
            ws = torch.empty(lib.gi_lpips_workspace_bytes(hd) + 256, dtype=torch.uint8, device=dev)
            off = (-ws.data_ptr()) % 256
            B.check(lib.gi_lpips_bind(hd, B.ptr(self.flat), ws.data_ptr() + off, ws.numel() - off))
            gws = None
            if self.grad:
                gws = torch.empty(lib.gi_lpips_grad_workspace_bytes(hd) + 256, dtype=torch.uint8, device=dev)
                goff = (-gws.data_ptr()) % 256
                B.check(lib.gi_lpips_bind_grad(hd, gws.data_ptr() + goff, gws.numel() - goff))
            self._handles[key] = (hd, (ws, gws))
            self._dirty = True
        hd = self._handles[key][0]
        if self._dirty:
            for h2, _ in self._handles.values():
                B.check(B.lib().gi_lpips_sync_weights(h2))
            self._dirty = False
        return hd

    def _check(self, x):
        if x.dim() == 4 and x.shape[1] == 3:
            raise B.BackendError("LPIPS takes grey (n,1,H,W) images (they are repeated over the three input channels); colour (n,3,H,W) "
                                 "inputs are not supported")
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 1:
            raise B.BackendError("LPIPS takes (n,1,H,W) float32 tensors on the gfx950 device")
        if self.flat.device != x.device:
            raise B.BackendError("LPIPS parameters live on %s, input on %s: call .to(device)" % (self.flat.device, x.device))

    @torch.no_grad()
    def distance(self, a, b, per_layer=False):
        """(n,) float32 device tensor of LPIPS(a[i], b[i]); per_layer: also the (5, n) terms. Batches of more than max_pairs run in
        chunks. The first layer, the tap kernels and the final sums give a pair the same bits whatever the chunk it is in; the twelve
        3x3 convolutions do so as long as every chunk size is served by the same implicit-GEMM kernel, which is NOT guaranteed: the
        dispatch takes the igemm8 family only from 512 workgroups up, and the grid grows with the chunk (at 256x256 with max_pairs=16
        a remainder chunk runs conv4_x on another family than a full one). Same-size chunks always agree bit for bit."""
        self._check(a)
        self._check(b)
        if a.shape != b.shape:
            raise ValueError(f"LPIPS.distance: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
        a, b = a.detach().contiguous(), b.detach().contiguous()
        n = a.shape[0]
        hd = self._handle(a.shape[2], a.shape[3], a.device)
        out = torch.empty(n, dtype=torch.float32, device=a.device)
        layers = torch.empty(5, n, dtype=torch.float32, device=a.device) if per_layer else None
        for i in range(0, n, self.max_pairs):
            k = min(self.max_pairs, n - i)
            part = torch.empty(5, k, dtype=torch.float32, device=a.device) if per_layer else None
            B.check(B.lib().gi_lpips_distance(hd, B.ptr(a[i:i + k]), B.ptr(b[i:i + k]), k, B.ptr(out[i:i + k]), B.ptr(part)))
            if per_layer:
                layers[:, i:i + k] = part
        return (out, layers) if per_layer else out

    @torch.no_grad()
    def distance_and_grad(self, a, b, gscale=1.0, per_layer=False):
        """(d, grad): d as `distance` (the same kernels: the same bits as a grad=False model gives for chunks of the same size), grad
        (n,1,H,W) float32 with grad[i] = gscale * d d[i] / d a[i]; b is a constant. Chunked by max_pairs; every image carries its own
        power-of-two scale through the fp16 backward, so its gradient does not depend on what else is in its chunk beyond the kernel
        dispatch caveat of `distance`. Needs LPIPS(grad=True)."""
        if not self.grad:
            raise B.BackendError("LPIPS.distance_and_grad needs LPIPS(grad=True): the backward keeps the feature maps in a second workspace")
        self._check(a)
        self._check(b)
        if a.shape != b.shape:
            raise ValueError(f"LPIPS.distance_and_grad: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
        a, b = a.detach().contiguous(), b.detach().contiguous()
        n = a.shape[0]
        hd = self._handle(a.shape[2], a.shape[3], a.device)
        out = torch.empty(n, dtype=torch.float32, device=a.device)
        grad = torch.empty_like(a)
        layers = torch.empty(5, n, dtype=torch.float32, device=a.device) if per_layer else None
        for i in range(0, n, self.max_pairs):
            k = min(self.max_pairs, n - i)
            part = torch.empty(5, k, dtype=torch.float32, device=a.device) if per_layer else None
            B.check(B.lib().gi_lpips_distance_grad(hd, B.ptr(a[i:i + k]), B.ptr(b[i:i + k]), k, B.ptr(out[i:i + k]), B.ptr(part),
                                                   B.ptr(grad[i:i + k]), float(gscale)))
            if per_layer:
                layers[:, i:i + k] = part
        return (out, grad, layers) if per_layer else (out, grad)

    @torch.no_grad()
    def grad_tap(self, tap, like):
        """Gradient w.r.t. the post-ReLU map of tap 0..4 of the last distance_and_grad chunk on the handle `like` (its input `a`) ran on,
        as (n,C,h,w) float32, gscale not applied (parity checks); like.shape[0] <= max_pairs."""
        if not self.grad:
            raise B.BackendError("LPIPS.grad_tap needs LPIPS(grad=True)")
        hd = self._handle(like.shape[2], like.shape[3], like.device)
        s = 1 << tap
        out = torch.empty(like.shape[0], self.TAP_CHANNELS[tap], like.shape[2] // s, like.shape[3] // s, dtype=torch.float32, device=like.device)
        B.check(B.lib().gi_lpips_grad_tap(hd, int(tap), B.ptr(out)))
        return out

    @torch.no_grad()
    def features(self, x, tap):
        """Feature map of tap 0..4 (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3) as (n,C,h,w) float32; n <= max_pairs."""
        self._check(x)
        if x.shape[0] > self.max_pairs:
            raise B.BackendError("LPIPS(max_pairs=%d).features got a batch of %d" % (self.max_pairs, x.shape[0]))
        x = x.detach().contiguous()
        hd = self._handle(x.shape[2], x.shape[3], x.device)
        s = 1 << tap
        out = torch.empty(x.shape[0], self.TAP_CHANNELS[tap], x.shape[2] // s, x.shape[3] // s, dtype=torch.float32, device=x.device)
        B.check(B.lib().gi_lpips_features(hd, B.ptr(x), x.shape[0], tap, B.ptr(out)))
        return out

    def forward(self, a, b):
        return self.distance(a, b)

    def __del__(self):
        try:
            for hd, _ in self._handles.values():
                B.lib().gi_lpips_destroy(hd)
        except Exception:
            pass
