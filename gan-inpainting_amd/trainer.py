"""Per-batch step schedules of the reference's training loops, driven straight through the C-ABI
(no autograd graph, preallocated buffers, no host synchronisation inside a step):

    MinimaxStep   experiment_list/minimaxgan_l1.py:110-173 (recon='rmse': minimaxgan_rmse.py)
    WGANStep      experiment_list/wgan_l1.py:110-186 / wgan_rmse.py  (weight clipping :151-153)
    DualDStep     experiment_list/experiment1_global_local_D.py:139-200

Scalar losses stay on the device (1-element tensors); the plugins read them back at their own
logging cadence. With a GradSync (parallel.py) every optimizer step is preceded by a bucketed
all-reduce of that network's flat gradient buffer.
"""
import torch

from . import backend as B
from . import optim
from .lib.models import util


class _Ops:
    """Thin allocation-free wrappers over the elementwise / loss entry points."""

    def __init__(self, device):
        self.dev = torch.device(device)
        self.scratch = torch.empty(2048, dtype=torch.float64, device=self.dev).view(torch.float32)   # 4096 floats, 8-byte aligned

    @property
    def ctx(self):
        return B.get_ctx(self.dev)

    def mask_apply(self, ground, mask, mask_c, masked, do_ceil):
        B.check(B.lib().gi_mask_apply(self.ctx, B.ptr(ground), B.ptr(mask), B.ptr(mask_c), B.ptr(masked), ground.numel(),
                                      1 if do_ceil else 0))

    def composite(self, masked, gen, mask_c, out):
        B.check(B.lib().gi_mask_composite(self.ctx, B.ptr(masked), B.ptr(gen), B.ptr(mask_c), B.ptr(out), out.numel()))

    def mul(self, a, b, out):
        B.check(B.lib().gi_mul(self.ctx, B.ptr(a), B.ptr(b), B.ptr(out), out.numel()))

    def add(self, a, b, out, alpha=1.0):
        B.check(B.lib().gi_add(self.ctx, B.ptr(a), B.ptr(b), B.ptr(out), out.numel(), float(alpha)))

    def adv(self, pred, kind, target, loss_out, grad, gscale=1.0):
        B.check(B.lib().gi_loss_adv(self.ctx, B.ptr(pred), pred.numel(), kind, float(target), B.ptr(loss_out), B.ptr(grad),
                                    float(gscale)))

    def adv_pair(self, pred2, n, kind, t_a, t_b, loss_a, loss_b, grad2, gs_a=1.0, gs_b=1.0):
        """adv() of both halves of a stacked [a | b] prediction vector in one launch (gi_loss_adv_pair)."""
        if not hasattr(B.lib(), "gi_loss_adv_pair"):      # an older build loaded through GI_LIB_PATH for an A/B run
            self.adv(pred2[:n], kind, t_a, loss_a, grad2[:n], gs_a)
            self.adv(pred2[n:], kind, t_b, loss_b, grad2[n:], gs_b)
            return
        B.check(B.lib().gi_loss_adv_pair(self.ctx, B.ptr(pred2), int(n), kind, float(t_a), float(t_b), B.ptr(loss_a), B.ptr(loss_b),
                                         B.ptr(grad2), float(gs_a), float(gs_b)))

    def recon(self, kind, a, b, loss_out, grad, gscale=1.0):
        lib = B.lib()
        if kind == "l1":
            B.check(lib.gi_loss_l1(self.ctx, B.ptr(a), B.ptr(b), a.numel(), B.ptr(loss_out), B.ptr(grad), float(gscale), B.ptr(self.scratch)))
        elif kind == "rmse":
            B.check(lib.gi_loss_rmse(self.ctx, B.ptr(a), B.ptr(b), a.numel(), 1e-16, B.ptr(loss_out), B.ptr(grad), float(gscale),
                                     B.ptr(self.scratch)))
        else:
            raise ValueError(kind)

    def local(self, kind, yhat, y, mask, loss_out, grad, gscale=1.0):
        """LocalLoss (loss.py:24-47): kind 'l1' | 'mse' | 'rmse' (the sqrt extension); gradient w.r.t. yhat."""
        code = {"l1": 0, "mse": 1, "rmse": 2}[kind]
        B.check(B.lib().gi_loss_local(self.ctx, B.ptr(yhat), B.ptr(y), B.ptr(mask), yhat.numel(), code, B.ptr(loss_out), B.ptr(grad),
                                      float(gscale), B.ptr(self.scratch)))

    def tv(self, img, weight, loss_out, grad, gscale=1.0):
        n, c, h, w = img.shape
        B.check(B.lib().gi_loss_tv(self.ctx, B.ptr(img), n * c, h, w, float(weight), B.ptr(loss_out), B.ptr(grad), float(gscale),
                                   B.ptr(self.scratch)))

    def cross_entropy(self, logits, labels, class_weight, loss_out2, grad, gscale=1.0):
        import ctypes as C
        n, k = logits.shape[0], logits.shape[1]
        hw = logits.numel() // (n * k)
        cw = (C.c_float * k)(*[float(v) for v in class_weight]) if class_weight is not None else None
        B.check(B.lib().gi_loss_cross_entropy(self.ctx, B.ptr(logits), B.ptr(labels), n, k, hw, C.cast(cw, C.c_void_p) if cw is not None else None,
                                              -100, B.ptr(loss_out2), B.ptr(grad), float(gscale), B.ptr(self.scratch)))


BCE, LSGAN, MEAN = 0, 1, 2


class _StepBase:
    recon_weight = 1.0      # largest multiplier on a mean-reduced reconstruction loss (lambda)
    auto_loss_scale = True  # fp16 only: pick per-network loss scales from the batch geometry

    def __init__(self, net_G, nets_D, device, sync=None, ema_G=None, diffaug=None):
        self.G, self.Ds = net_G, list(nets_D)
        # differentiable augmentation of everything a discriminator sees (lib/models/augment.py): None, a policy
        # string or a DiffAugment. _aug_step counts the batches this object has processed: it keys the draws
        if diffaug is not None and not hasattr(diffaug, "into"):
            from .lib.models.augment import DiffAugment
            diffaug = DiffAugment(diffaug)
        self.aug = diffaug
        self._aug_step = 0
        # optim.EMA of the generator (or None): updated right after every generator update, on its stream. It may also be set
        # after construction, which under data parallelism is after the parameter broadcast below
        self.ema_G = ema_G
        self._loaded_scales = self._loaded_L = None
        self.ops = _Ops(device)
        self.sync = sync
        self._shape = None
        for n in [net_G] + self.Ds:
            n.train()
            # inside a step object parameters only change through the package's optimizers / clamp, which
            # mark the network dirty: re-derive packed weights once per update instead of once per forward
            n.always_sync = False
        if sync is not None:
            sync.prepare(net_G.device)
            sync.broadcast_parameters([net_G] + self.Ds)    # replicas start identical whatever the ranks' RNG state
            if hasattr(net_G, "set_dropout_seed"):          # ... but draw their own dropout masks
                net_G.set_dropout_seed(0x5EED0000 + 1000 * sync.rank)

    def _bind_optimizers(self, *opts):
        self._opts = opts
        if self.sync is not None:
            for o in opts:
                o.grad_scale = self.sync.grad_scale()   # SUM all-reduce -> mean gradient

    def _buffers(self, ground):
        if self._shape != tuple(ground.shape):
            self._shape = tuple(ground.shape)
            mk = lambda: torch.empty_like(ground)  # noqa: E731
            self.mask_c, self.masked, self.inpainted = mk(), mk(), mk()
            self.g_adv, self.g_rec, self.g_gen, self.tmp1, self.tmp2 = mk(), mk(), mk(), mk(), mk()
            n, _, h, w = ground.shape
            # prediction / its gradient as the discriminator returns it: (n, 1), or (2n, 1) for DCGANDiscriminator
            self.dpred = torch.empty(self.Ds[0]._output_shape(n, h, w), dtype=torch.float32, device=ground.device)
            if self.aug is not None:    # T(real) / T(generated) of the un-stacked critic calls, T2(inpainted) of the generator update
                self.aug_a, self.aug_b = mk(), mk()
            self.L = {}
            if self.auto_loss_scale:
                self._pick_loss_scales(ground)
            self._apply_loaded_state()

    def _pick_loss_scales(self, ground):
        """fp16 backward: the gradient entering the generator is ~ lambda / (N*H*W) per pixel (mean-
        reduced L1/RMSE), the one entering a discriminator ~ 1/N per sample. Scale each network so
        these land around 2^-5 in fp16 (normal range 6e-5 .. 65504); the library removes the scale
        when it writes the fp32 parameter gradients / the input gradient."""
        import math
        n, _, h, w = ground.shape
        if self.G._dtype == B.GI_F16:
            g0 = self.recon_weight / float(n * h * w)
            self.G.set_loss_scale(min(65536.0, max(1.0, 2.0 ** round(math.log2(0.03 / g0)))))
        for d in self.Ds:
            if d._dtype == B.GI_F16:
                d.set_loss_scale(min(65536.0, 64.0 * n))

    # ---- resumable training ----
    def _nets(self):
        return [self.G] + self.Ds

    def state_dict(self):
        """What the step carries across batches and a result depends on: the networks' loss scales (poll_overflow halves them);
        the loss scalars (a WGAN step returns the generator's terms of its LAST generator update on every batch, and the epoch
        loop averages what it is handed: the first batches of an epoch see the previous epoch's values); plus whatever a
        subclass adds in _extra_state. Reads the device: call it with the step's streams idle."""
        return {"loss_scales": [float(n._loss_scale) for n in self._nets()],
                "losses": {k: v.detach().float().cpu().clone() for k, v in getattr(self, "L", {}).items()},
                "extra": self._extra_state()}

    def load_state_dict(self, sd):
        if len(sd["loss_scales"]) != len(self._nets()):
            raise B.BackendError(f"step state holds {len(sd['loss_scales'])} loss scales, this step has {len(self._nets())} networks")
        # kept until the first batch: _buffers picks the scales from the batch geometry there, and the loaded ones must survive it
        self._loaded_scales = [float(v) for v in sd["loss_scales"]]
        for n, v in zip(self._nets(), self._loaded_scales):
            n.set_loss_scale(v)
        self._loaded_L = dict(sd.get("losses") or {})
        self._shape = None              # the next batch goes through _buffers, which applies both
        self._load_extra_state(sd.get("extra") or {})

    def _apply_loaded_state(self):
        """First batch after load_state_dict, from _buffers: the loaded loss scales over the ones just picked, the loaded loss
        scalars into the fresh dict."""
        if self._loaded_scales is not None:
            for n, v in zip(self._nets(), self._loaded_scales):
                n.set_loss_scale(v)
            self._loaded_scales = None
        if self._loaded_L:
            for k, v in self._loaded_L.items():
                self.L[k] = v.to(self.ops.dev, torch.float32).view(1).clone()
            torch.cuda.synchronize(self.ops.dev)     # once per resume: the side stream writes these too
        self._loaded_L = None

    def _extra_state(self):
        return {} if self.aug is None else {"diffaug_step": int(self._aug_step)}

    def _load_extra_state(self, d):
        if self.aug is not None and "diffaug_step" in d:
            self._aug_step = int(d["diffaug_step"])

    # ---- differentiable augmentation: key = ((step * 4 + call) << 32) | (rank * n + row) ----
    def _aug_into(self, x, call, out):
        """out = T_call(x) with this batch's draws, on the current stream."""
        n = x.shape[0]
        self.aug.into(x, out, self._aug_step, call, (self.sync.rank if self.sync is not None else 0) * n)
        return out

    def _aug_adjoint(self, dy, call, out):
        n = dy.shape[0]
        self.aug.adjoint_into(dy, out, self._aug_step, call, (self.sync.rank if self.sync is not None else 0) * n)
        return out

    def _d_for_g(self, net, inp, kind, target, name, gscale=1.0):
        """The generator update's critic call: loss into L[name], returns d(loss)/d(inp). With augmentation the critic sees
        T2(inp) and its input gradient goes back through the adjoint."""
        x = inp if self.aug is None else self._aug_into(inp, 2, self.aug_a)
        p, t = self._fwd(net, x)
        self.ops.adv(p, kind, target, self._loss(name), self.dpred, gscale)
        d = self._bwd(net, t, self.dpred, True, False)
        return d if self.aug is None else self._aug_adjoint(d, 2, self.g_adv)

    def _step_G(self, opt):
        """_step of the generator's optimizer, then the moving average of its parameters (same stream, no synchronisation)."""
        self._step(opt)
        if self.ema_G is not None:
            self.ema_G.update(opt)

    # ---- stream contract for readers of the step's results (plugins: loss accumulation, gradient-flow statistics) ----
    def side_stream(self):
        """The HIP stream the discriminator side of the step runs on, or None when everything is on the caller's."""
        return None

    def side_keys(self):
        """Keys of the loss dict whose values (and the discriminators' gradient buffers) are produced on side_stream()."""
        return ()

    def sync_for_logging(self):
        """Make the caller's stream wait for everything the step has issued on its side stream, so that losses,
        discriminator gradients and overflow flags can be read from the caller's stream."""

    def poll_overflow(self, logger=None):
        """fp16 only, call at logging cadence: when an optimizer skipped updates because its gradients held
        inf/NaN, halve the loss scale of its networks (they re-derive it from the batch geometry otherwise)."""
        self.sync_for_logging()
        out = 0
        for opt in getattr(self, "_opts", ()):
            new = opt.poll_skipped()
            if new:
                out += new
                for net in opt.nets:
                    if net._dtype == B.GI_F16:
                        net.set_loss_scale(max(1.0, net._loss_scale / 2.0))
                        if logger:
                            logger.info("fp16 overflow: %d update(s) of %s skipped, loss scale -> %g", new, type(net).__name__, net._loss_scale)
        return out

    def _loss(self, name):
        if name not in self.L:
            self.L[name] = torch.zeros(1, dtype=torch.float32, device=self.ops.dev)
        return self.L[name]

    def _reduce(self, net):
        """Start the all-reduce of a network's whole gradient buffer (no overlap with its backward); _step waits for it."""
        if self.sync is not None:
            self.sync.launch(net.flat_grads())

    def _step(self, opt):
        """Optimizer update of the networks of `opt`. The gradient exchange is awaited HERE, as late as possible: whatever
        the stream issued between the backward and this call (on critic-only batches of the overlapped WGAN step: nothing
        on the critic's stream, while the main stream is already in the next batch's generator forward) overlaps it."""
        if self.sync is not None and self.sync.world > 1:
            for net in opt.nets:
                flat = net.flat_grads()
                self.sync.wait(flat.device if flat.is_cuda else None, flat=flat)
        opt.step()

    def _bwd_G(self, gtok, dy):
        """Generator backward; with a GradSync the gradients start their all-reduce in completion order while the
        rest of the backward is still being computed: decoder, then the inner encoder levels (d7 .. d5, 82 % of the
        encoder's gradients), then the outer ones."""
        if self.sync is None or self.sync.world == 1:
            return self._bwd(self.G, gtok, dy, False, True)
        G, lib = self.G, B.lib()
        if G._slot_gen[gtok[0]] != gtok[1]:
            raise B.BackendError("generator activations were overwritten before their backward")
        flat = G.flat_grads()
        split, split2 = lib.gi_net_phase_split(G._handle), lib.gi_net_phase_split2(G._handle)
        B.check(lib.gi_net_backward_phase(G._handle, gtok[0], B.ptr(dy), None, 1, 1))
        self.sync.launch(flat, split, flat.numel())
        B.check(lib.gi_net_backward_phase(G._handle, gtok[0], B.ptr(dy), None, 1, 3))
        self.sync.launch(flat, split2, split)
        B.check(lib.gi_net_backward_phase(G._handle, gtok[0], B.ptr(dy), None, 1, 4))
        self.sync.launch(flat, 0, split2)       # awaited by _step(optG)

    def _d_pair(self, net, real, fake, kind, t_real, t_fake, name_real, name_fake, gs_real=1.0, gs_fake=1.0, synced=False, x2=None,
                real_done=False):
        """A discriminator's two calls of a batch, D(real) and D(fake), as ONE [real | fake] batch whose BatchNorm
        layers are evaluated per half (gi_net_set_bn_groups): per image the reference's arithmetic, half the
        launches, one weight-gradient GEMM over both halves. Losses go to L[name_*], gradients accumulate."""
        o, n = self.ops, real.shape[0]
        bufs = self.__dict__.setdefault("_pair_bufs", {})
        key = (id(net), tuple(real.shape))
        if key not in bufs:
            bufs[key] = (torch.empty((2 * n,) + tuple(real.shape[1:]), dtype=torch.float32, device=real.device),
                         torch.empty(net._output_shape(2 * n, real.shape[2], real.shape[3]), dtype=torch.float32, device=real.device))
        own, dp2 = bufs[key]
        if x2 is None:
            x2 = own
        if self.aug is not None:                      # T0(real) | T1(fake), written straight into the pair buffer
            if not real_done:
                self._aug_into(real, 0, x2[:n])
            self._aug_into(fake, 1, x2[n:])
        else:
            if not real_done:                             # (the caller may have copied the real half already, ahead of a wait)
                x2[:n].copy_(real)
            if fake.data_ptr() != x2[n:].data_ptr():      # the caller may have produced `fake` in the pair buffer already
                x2[n:].copy_(fake)
        self._pair = x2
        p, t = self._fwd(net, x2, bn_groups=2)
        o.adv_pair(p, p.shape[0] // 2, kind, t_real, t_fake, self._loss(name_real), self._loss(name_fake), dp2, gs_real, gs_fake)
        if synced:
            self._bwd_D_synced(net, t, dp2)
        else:
            self._bwd(net, t, dp2, False, True)

    def _bwd_D_synced(self, net, tok, dy):
        """Critic backward + gradient all-reduce: the conv4 block and the head (8.5 of 11 MB) are reduced while
        conv3 .. conv1 are still in their backward; the optimizer step (_step) waits for both ranges."""
        lib = B.lib()
        if net._slot_gen[tok[0]] != tok[1]:
            raise B.BackendError("critic activations were overwritten before their backward")
        dy = dy.contiguous()
        if net._slot_groups[tok[0]] != net._groups_set:
            B.check(lib.gi_net_set_bn_groups(net._handle, net._slot_groups[tok[0]]))
            net._groups_set = net._slot_groups[tok[0]]
        flat = net.flat_grads()
        split = lib.gi_net_phase_split(net._handle)
        B.check(lib.gi_net_backward_phase(net._handle, tok[0], B.ptr(dy), None, 1, 1))
        self.sync.launch(flat, split, flat.numel())
        B.check(lib.gi_net_backward_phase(net._handle, tok[0], B.ptr(dy), None, 1, 2))
        self.sync.launch(flat, 0, split)        # awaited by _step(optD)

    @staticmethod
    def _fwd(net, x, bn_groups=1):
        y, slot, gen = net._forward_raw(x, bn_groups) if bn_groups != 1 else net._forward_raw(x)
        return y, (slot, gen)

    @staticmethod
    def _bwd(net, tok, dy, need_dx, need_wgrad):
        return net._backward_raw(tok[0], tok[1], dy, need_dx, need_wgrad)


class MinimaxStep(_StepBase):
    def __init__(self, net_G, net_D, opt_G, opt_D, recon="l1", sync=None, stacked=True, ema_G=None, diffaug=None, lpips=None,
                 lpips_weight=0.0):
        if lpips is not None or lpips_weight:
            raise B.BackendError("MinimaxStep takes no LPIPS term: only the WGAN steps (WGANStep, WGANPerceptualStep) are pinned "
                                 "against an oracle step with an extra generator loss")
        super().__init__(net_G, [net_D], net_G.device, sync, ema_G, diffaug)
        self.D, self.optG, self.optD, self.recon = net_D, opt_G, opt_D, recon
        self.stacked = stacked      # D(ground) | D(inpainted) as one batch with per-half BatchNorm (see _d_pair)
        self._bind_optimizers(opt_G, opt_D)

    @torch.no_grad()
    def __call__(self, ground, mask):
        o = self.ops
        self._buffers(ground)
        o.mask_apply(ground, mask, self.mask_c, self.masked, True)             # :114-117
        gen, gtok = self._fwd(self.G, self.masked)                              # :119
        o.composite(self.masked, gen, self.mask_c, self.inpainted)             # :122
        # ---- D step :129-148
        self.optD.zero_grad()
        if self.stacked:
            self._d_pair(self.D, ground, self.inpainted, BCE, 1.0, 0.0, "d_loss_real", "d_loss_fake")
        else:
            real, fake = ground, self.inpainted
            if self.aug is not None:
                real, fake = self._aug_into(ground, 0, self.aug_a), self._aug_into(self.inpainted, 1, self.aug_b)
            p, t = self._fwd(self.D, real)
            o.adv(p, BCE, 1.0, self._loss("d_loss_real"), self.dpred)
            self._bwd(self.D, t, self.dpred, False, True)
            p, t = self._fwd(self.D, fake)
            o.adv(p, BCE, 0.0, self._loss("d_loss_fake"), self.dpred)
            self._bwd(self.D, t, self.dpred, False, True)
        self._reduce(self.D)
        self._step(self.optD)
        # ---- G step :154-173 (D frozen: input gradient only)
        self.optG.zero_grad()
        d_adv = self._d_for_g(self.D, self.inpainted, BCE, 1.0, "g_adv")
        o.recon(self.recon, self.inpainted, ground, self._loss("recon"), self.g_rec)
        o.add(d_adv, self.g_rec, self.tmp1)
        o.mul(self.tmp1, self.mask_c, self.g_gen)                              # d(inpainted)/d(gen) = mask
        self._bwd_G(gtok, self.g_gen)
        self._step_G(self.optG)
        self._aug_step += 1
        return self.L


class WGANStep(_StepBase):
    """clip > 0 applies the reference's weight clipping after the critic update. If opt_D is this
    package's RMSprop its `clamp` is set so the clip is fused into the optimizer kernel."""

    def __init__(self, net_G, net_D, opt_G, opt_D, recon="l1", clip=0.01, sync=None, gp_lambda=0.0, overlap=False, stacked=True,
                 ema_G=None, diffaug=None, lpips=None, lpips_weight=0.0):
        super().__init__(net_G, [net_D], net_G.device, sync, ema_G, diffaug)
        self.D, self.optG, self.optD, self.recon, self.clip = net_D, opt_G, opt_D, recon, clip
        # lpips (lib.lpips.LPIPS(grad=True), NOT in the reference): lpips_weight * mean_i LPIPS(inpainted_i, ground_i) joins the
        # generator's loss with its analytic image gradient (csrc/lpips.hip). None: nothing is allocated or launched
        self.lpips, self.lpips_weight = lpips, float(lpips_weight)
        if lpips is not None and not getattr(lpips, "grad", False):
            raise B.BackendError("WGANStep(lpips=...) needs lib.lpips.LPIPS(grad=True)")
        self._lpips_fold, self._lpips_scaled_for = 0.0, None
        # stacked=True: the critic's two calls of a batch, D(ground) and D(inpainted) (wgan_l1.py:134-135), run as ONE
        # 2n batch with independent BatchNorm statistics per half (gi_net_set_bn_groups): same arithmetic per
        # image, half the launches, and one weight-gradient GEMM over both halves instead of two accumulating ones.
        self.stacked = stacked
        # overlap=True: the critic runs on a side HIP stream. Its real-image forward/backward does not depend
        # on the generator forward, and in critic-only batches the next batch's generator forward does not
        # depend on this batch's critic update, so the two networks' small / latency-bound kernels fill each
        # other's idle CUs. Results are identical (same kernels, same order per network).
        self.overlap = overlap
        if overlap:
            self._sD = torch.cuda.Stream(device=net_G.device)
            net_D._release_handle()          # the handle launches on the stream that is current when it is created
            self._inp2 = [None, None]
            self._inp1 = [None, None]       # with augmentation: the plain composite (the pair buffer holds its transform)
            self._evD = [None, None]
            self._k = 0
        # True: `ground` / `mask` were produced before the previous step was issued (resident in HBM, the
        # benchmark's contract), so the side stream need not wait for the main stream's pending work (the
        # previous batch's generator backward) before the critic's real-image pass.
        self.inputs_resident = False
        # gp_lambda > 0: WGAN-GP extension (BASELINE config 2) instead of the reference's weight clipping
        self.gp_lambda = gp_lambda
        if gp_lambda > 0:
            self.clip = clip = 0.0
        self._fused_clip = isinstance(opt_D, optim.RMSprop)
        if self._fused_clip:
            opt_D.clamp = clip
        self._bind_optimizers(opt_G, opt_D)

    @torch.no_grad()
    def _call_overlapped(self, ground, mask, update_g):
        o = self.ops
        self._d_synced = False
        self._buffers(ground)
        main = torch.cuda.current_stream(ground.device)
        sD = self._sD
        k = self._k
        self._k ^= 1
        if self._inp2[k] is None or self._inp2[k].shape[0] != 2 * ground.shape[0] or self._inp2[k].shape[1:] != ground.shape[1:]:
            # [ground | inpainted] of the stacked critic pass: the composite writes its half in place
            self._inp2[k] = torch.empty((2 * ground.shape[0],) + tuple(ground.shape[1:]), dtype=ground.dtype, device=ground.device)
        inp = self._inp2[k][ground.shape[0]:]
        if self.aug is not None:
            # the pair buffer takes T0(ground) | T1(inpainted) on the side stream; the composite goes to a plain buffer, which the
            # reconstruction terms, the caller (metrics) and the transforms read. Two of them for the same reason as the pair
            if self._inp1[k] is None or self._inp1[k].shape != ground.shape:
                self._inp1[k] = torch.empty_like(ground)
            inp = self._inp1[k]
        # the side stream reads the caller's `ground` (critic real half, gradient penalty): tell the caching allocator,
        # or a per-batch `ground` freed by the caller could be handed to the next batch's H2D copy while the critic
        # still reads it (critic-only batches never make the main stream wait for the side stream)
        ground.record_stream(sD)
        if self._evD[k] is not None:
            main.wait_event(self._evD[k])        # the critic pass that read this buffer two batches ago is done
        e0 = main.record_event()
        o.mask_apply(ground, mask, self.mask_c, self.masked, True)
        gen, gtok = self._fwd(self.G, self.masked)
        o.composite(self.masked, gen, self.mask_c, inp)
        e_inp = main.record_event()
        self.inpainted = inp
        d_adv = None
        with torch.cuda.stream(sD):
            if not self.inputs_resident:
                sD.wait_event(e0)
            self.optD.zero_grad()
            gp_real, gp_fake = ground, inp
            if self.stacked:
                # the real half of the pair: before the wait for the inpainted one
                if self.aug is not None:
                    self._aug_into(ground, 0, self._inp2[k][:ground.shape[0]])
                    gp_real, gp_fake = self._inp2[k][:ground.shape[0]], self._inp2[k][ground.shape[0]:]
                else:
                    self._inp2[k][:ground.shape[0]].copy_(ground)
                sD.wait_event(e_inp)
                self._critic_stacked(ground, inp, x2=self._inp2[k], real_done=True)
            else:
                if self.aug is not None:
                    gp_real = self._aug_into(ground, 0, self.aug_a)
                pr, tr = self._fwd(self.D, gp_real)
                o.adv(pr, MEAN, 0.0, self._loss("d_loss_real"), self.dpred, +1.0)
                self._bwd(self.D, tr, self.dpred, False, True)
                sD.wait_event(e_inp)
                if self.aug is not None:
                    gp_fake = self._aug_into(inp, 1, self.aug_b)
                pf, tf = self._fwd(self.D, gp_fake)
                o.adv(pf, MEAN, 0.0, self._loss("d_loss_fake"), self.dpred, -1.0)
                self._bwd(self.D, tf, self.dpred, False, True)
            if self.gp_lambda > 0:      # with augmentation: between the two augmented halves
                self.L["gp"] = self.D.gradient_penalty(gp_real, gp_fake, getattr(self, "gp_eps", None), self.gp_lambda).view(1)
            if not self._d_synced:
                self._reduce(self.D)
            self._step(self.optD)
            if self.clip > 0 and not self._fused_clip:
                util.clamp_parameters(self.D, -self.clip, self.clip)
            if update_g:
                d_adv = self._d_for_g(self.D, inp, MEAN, 0.0, "g_adv", +1.0)
            self._evD[k] = sD.record_event()
        if update_g:
            # before the wait - the main stream has nothing else to do while the critic runs: clearing the generator's gradients
            # and every loss term that depends on (inpainted, ground) only, i.e. all but the adversarial one
            self.optG.zero_grad()
            g_other = self._g_terms(inp, ground)
            main.wait_event(self._evD[k])
            d_adv.record_stream(main)
            o.add(d_adv, g_other, self.tmp1)
            o.mul(self.tmp1, self.mask_c, self.g_gen)
            self._bwd_G(gtok, self.g_gen)
            self._step_G(self.optG)
        self._aug_step += 1
        return self.L

    def side_stream(self):
        return self._sD if self.overlap else None

    def side_keys(self):
        return ("d_loss_real", "d_loss_fake", "gp", "g_adv") if self.overlap else ()

    def sync_for_logging(self):
        if self.overlap:
            torch.cuda.current_stream(self.G.device).wait_stream(self._sD)

    @torch.no_grad()
    def __call__(self, ground, mask, update_g):
        if self.overlap:
            return self._call_overlapped(ground, mask, update_g)
        o = self.ops
        self._d_synced = False
        self._buffers(ground)
        o.mask_apply(ground, mask, self.mask_c, self.masked, True)
        gen, gtok = self._fwd(self.G, self.masked)                              # every batch, :119
        o.composite(self.masked, gen, self.mask_c, self.inpainted)
        self.optD.zero_grad()
        gp_real, gp_fake = ground, self.inpainted
        if self.stacked:
            self._critic_stacked(ground, self.inpainted)
            if self.aug is not None:
                gp_real, gp_fake = self._pair[:ground.shape[0]], self._pair[ground.shape[0]:]
        else:
            if self.aug is not None:
                gp_real, gp_fake = self._aug_into(ground, 0, self.aug_a), self._aug_into(self.inpainted, 1, self.aug_b)
            pr, tr = self._fwd(self.D, gp_real)                                     # :134
            pf, tf = self._fwd(self.D, gp_fake)                                     # :135
            o.adv(pr, MEAN, 0.0, self._loss("d_loss_real"), self.dpred, +1.0)       # backward(one)  :137-138
            self._bwd(self.D, tr, self.dpred, False, True)
            o.adv(pf, MEAN, 0.0, self._loss("d_loss_fake"), self.dpred, -1.0)       # backward(mone) :140-141
            self._bwd(self.D, tf, self.dpred, False, True)
        if self.gp_lambda > 0:      # with augmentation: between the two augmented halves
            self.L["gp"] = self.D.gradient_penalty(gp_real, gp_fake, getattr(self, "gp_eps", None), self.gp_lambda).view(1)
        if not self._d_synced:
            self._reduce(self.D)
        self._step(self.optD)                                                   # :147
        if self.clip > 0 and not self._fused_clip:
            util.clamp_parameters(self.D, -self.clip, self.clip)                # :151-153
        if update_g:                                                            # cadence :157-163 is the caller's
            self.optG.zero_grad()
            d_adv = self._d_for_g(self.D, self.inpainted, MEAN, 0.0, "g_adv", +1.0)
            o.add(d_adv, self._g_terms(self.inpainted, ground), self.tmp1)
            o.mul(self.tmp1, self.mask_c, self.g_gen)
            self._bwd_G(gtok, self.g_gen)
            self._step_G(self.optG)
        self._aug_step += 1
        return self.L

    def _g_terms(self, inp, ground):
        """_g_losses plus, with lpips set, the LPIPS term: records L["lpips_loss"], adds its image gradient to the other terms'
        (before the mask multiply of the caller)."""
        if self.lpips is None:
            return self._g_losses(inp, ground)
        refold = self.auto_loss_scale and self.G._dtype == B.GI_F16 and self._lpips_scaled_for != self._shape
        if refold:
            self.recon_weight -= self._lpips_fold
            self._lpips_fold = 0.0
        g = self._g_losses(inp, ground)
        n, _, h, w = inp.shape
        d, gl = self.lpips.distance_and_grad(inp, ground, gscale=self.lpips_weight / n)
        self.L["lpips_loss"] = (d.sum() * (self.lpips_weight / n)).view(1)
        if refold:
            # as WGANPerceptualStep does for its VGG-19 terms: the fp16 generator's loss scale assumes
            # ~ recon_weight / (N H W) per pixel; ONE host read at the first generator update of a batch geometry puts this term's
            # largest per-pixel gradient, in the same units, on top
            self._lpips_fold = float(gl.abs().max()) * n * h * w
            self.recon_weight += self._lpips_fold
            self._pick_loss_scales(ground)
            self._lpips_scaled_for = self._shape
        self.ops.add(g, gl, g)
        return g

    def _extra_state(self):
        st = super()._extra_state()
        if self.lpips is not None:
            st = dict(st, recon_weight=float(self.recon_weight), lpips_fold=float(self._lpips_fold),
                      lpips_scaled_for=None if self._lpips_scaled_for is None else list(self._lpips_scaled_for))
        return st

    def _load_extra_state(self, d):
        super()._load_extra_state(d)
        if self.lpips is not None and "lpips_fold" in d:
            self.recon_weight = float(d["recon_weight"])
            self._lpips_fold = float(d["lpips_fold"])
            self._lpips_scaled_for = None if d.get("lpips_scaled_for") is None else tuple(d["lpips_scaled_for"])

    def _critic_stacked(self, ground, inp, x2=None, real_done=False):
        """D(ground) and D(inpainted) of wgan_l1.py:134-141 as one [ground | inpainted] batch, BatchNorm per half;
        backward(one) / backward(mone) are the gradient scales +1 / -1."""
        synced = self.sync is not None and self.sync.world > 1 and self.gp_lambda <= 0
        self._d_pair(self.D, ground, inp, MEAN, 0.0, 0.0, "d_loss_real", "d_loss_fake", +1.0, -1.0, synced=synced, x2=x2,
                     real_done=real_done)
        self._d_synced = synced   # the all-reduce already overlapped the tail of the backward

    def _g_losses(self, inp, ground):
        """Every non-adversarial generator loss: records the scalars, returns d(sum)/d(inpainted)."""
        self.ops.recon(self.recon, inp, ground, self._loss("recon"), self.g_rec)
        return self.g_rec


class WGANPerceptualStep(WGANStep):
    """experiment_list/wgan_perceptual_style_faceparsing.py:136-232 (BASELINE config 5): the WGAN schedule with
        g_loss = g_adv + recon_global + recon_local + perceptual + style + face_parsing + tv          (:222)
    recon_global = RMSELoss(ground, inpainted) (:206), recon_local = LocalLoss RMSE on the mask (:207; the file adds
    an undefined `recon_loss`: the sum of the two terms it computes is the evident intent), perceptual / style =
    loss.perceptual_and_style_loss(weight_p = weight_s = 0.01) (:216; constants, the reference runs them under
    no_grad), face_parsing = 0.01 * CrossEntropy(w=[0,1.2,0.7,0.7])(segment_model(inpainted), segment) (:212-213,
    frozen eval network: input gradient only), tv = tv_loss(inpainted, 1) (:219).
    `vgg` (networks.VGG19Wrapper) and `segment_model` (frozen UnetGenerator(1,4,7,ngf=32)) are optional: a missing
    one drops its term (the pretrained weights of both are not redistributable / not available here).
    perceptual_grad=True (NOT the reference, which never back-propagates these two terms): their analytic image gradient
    (VGG19Wrapper(grad=True).perceptual_and_style_grad) joins the other generator terms."""

    def __init__(self, net_G, net_D, opt_G, opt_D, vgg=None, segment_model=None, weight_p=0.01, weight_s=0.01, weight_fp=0.01,
                 tv_weight=1.0, ce_weight=(0, 1.2, 0.7, 0.7), perceptual_grad=False, **kw):
        super().__init__(net_G, net_D, opt_G, opt_D, recon="rmse", **kw)
        self.recon_weight = 2.0
        self.perceptual_grad = bool(perceptual_grad)
        if self.perceptual_grad and not getattr(vgg, "grad", False):
            raise B.BackendError("WGANPerceptualStep(perceptual_grad=True) needs vgg=VGG19Wrapper(..., grad=True)")
        self._vgg_scaled_for = None
        self.vgg, self.weight_p, self.weight_s = vgg, weight_p, weight_s
        self.tv_weight, self.weight_fp, self.ce_weight = tv_weight, weight_fp, list(ce_weight)
        self.seg = getattr(segment_model, "phys", segment_model)      # EmbeddedUnetGenerator -> the physical network
        self.segment = None
        if self.seg is not None:
            self.seg.eval()
            for p in self.seg.parameters():
                p.requires_grad_(False)
            self._ce2 = torch.zeros(2, dtype=torch.float32, device=net_G.device)
            self._zero1 = torch.zeros(1, dtype=torch.float32, device=net_G.device)
            self._dseg = None

    def _extra_state(self):
        # perceptual_grad on an fp16 generator: the loss scale was picked once from the first generator update's VGG gradient
        return dict(super()._extra_state(), recon_weight=float(self.recon_weight),
                    vgg_scaled_for=None if self._vgg_scaled_for is None else list(self._vgg_scaled_for))

    def _load_extra_state(self, d):
        super()._load_extra_state(d)
        if "recon_weight" in d:
            self.recon_weight = float(d["recon_weight"])
            self._vgg_scaled_for = None if d.get("vgg_scaled_for") is None else tuple(d["vgg_scaled_for"])

    def __call__(self, ground, mask, update_g, segment=None):
        self.segment = segment
        return super().__call__(ground, mask, update_g)

    def _g_losses(self, inp, ground):
        o = self.ops
        o.recon("rmse", inp, ground, self._loss("recon_global"), self.g_rec)                   # :206
        o.local("rmse", inp, ground, self.mask_c, self._loss("recon_local"), self.tmp2)        # :207
        o.add(self.g_rec, self.tmp2, self.g_rec)
        o.tv(inp, self.tv_weight, self._loss("tv"), self.tmp2)                                 # :219
        o.add(self.g_rec, self.tmp2, self.g_rec)
        if self.vgg is not None and self.perceptual_grad:
            p, s, gv = self.vgg.perceptual_and_style_grad(inp, ground, self.weight_p, self.weight_s)
            self.L["perceptual"], self.L["style"] = p.view(1), s.view(1)
            if self.auto_loss_scale and self.G._dtype == B.GI_F16 and self._vgg_scaled_for != self._shape:
                # the fp16 generator's loss scale assumes ~ recon_weight / (N H W) per pixel; how much these terms add depends on
                # the feature network and the weights, not on the geometry: ONE host read at the first generator update of a batch
                # geometry puts their largest per-pixel gradient, in the same units, on top of the two RMSE terms
                n, _, h, w = inp.shape
                self.recon_weight = 2.0 + float(gv.abs().max()) * n * h * w
                self._pick_loss_scales(ground)
                self._vgg_scaled_for = self._shape
            o.add(self.g_rec, gv, self.g_rec)
        elif self.vgg is not None:                                                             # :216 (no gradient)
            p, s = self.vgg.perceptual_and_style(inp, ground, self.weight_p, self.weight_s)
            self.L["perceptual"], self.L["style"] = p.view(1), s.view(1)
        if self.seg is not None and self.segment is not None:                                  # :212-213
            import math
            n, _, h, w = inp.shape
            if self.seg._dtype == B.GI_F16:   # gradient entering the frozen network ~ weight_fp / (n*h*w) per logit
                self.seg.set_loss_scale(min(2.0 ** 24, 2.0 ** round(math.log2(0.03 * n * h * w / self.weight_fp))))
            y, tok = self._fwd(self.seg, inp)
            if self._dseg is None or self._dseg.shape != y.shape:
                self._dseg = torch.empty_like(y)
            o.cross_entropy(y, self.segment, self.ce_weight, self._ce2, self._dseg, self.weight_fp)
            o.add(self._zero1, self._ce2[:1], self._loss("face_parsing"), self.weight_fp)
            dx = self._bwd(self.seg, tok, self._dseg, True, False)
            o.add(self.g_rec, dx, self.g_rec)
        return self.g_rec


def wgan_update_g(batch_index, g_iter_count, update_g_every=5):
    """G-update cadence of wgan_l1.py:157-163."""
    period = 140 if (g_iter_count < 25 or g_iter_count % 500 == 0) else update_g_every
    return batch_index % period == 0 and batch_index > 0


class DualDStep(_StepBase):
    """G step first, LSGAN losses, global + local (mask * x) discriminators, mask not ceil-ed,
    output not composited, one optimizer over both discriminators (:123)."""

    def __init__(self, net_G, net_Dg, net_Dl, opt_G, opt_D, lam1=300.0, lam2=300.0, sync=None, stacked=True, ema_G=None, diffaug=None,
                 lpips=None, lpips_weight=0.0):
        if lpips is not None or lpips_weight:
            raise B.BackendError("DualDStep takes no LPIPS term: only the WGAN steps (WGANStep, WGANPerceptualStep) are pinned "
                                 "against an oracle step with an extra generator loss")
        if diffaug is not None:
            # the local critic looks at mask * x: whether it shares the global critic's transform is undecided
            raise B.BackendError("DualDStep does not support diffaug")
        super().__init__(net_G, [net_Dg, net_Dl], net_G.device, sync, ema_G)
        self.stacked = stacked      # each discriminator's real | fake calls as one batch with per-half BatchNorm
        self.Dg, self.Dl, self.optG, self.optD, self.lam1, self.lam2 = net_Dg, net_Dl, opt_G, opt_D, lam1, lam2
        self.recon_weight = max(lam1, lam2)
        self._bind_optimizers(opt_G, opt_D)

    @torch.no_grad()
    def __call__(self, ground, mask):
        o = self.ops
        self._buffers(ground)
        o.mask_apply(ground, mask, None, self.masked, False)                    # :144
        self.optG.zero_grad()
        gen, gtok = self._fwd(self.G, self.masked)                              # :154
        self.gen = gen                                                          # the reference's `inpainted` (:154, metric at :209)
        # D_global(inpainted), D_local(mask*inpainted) with frozen Ds :156-157
        p, t = self._fwd(self.Dg, gen)
        o.adv(p, LSGAN, 1.0, self._loss("g_adv_global"), self.dpred)
        d1 = self._bwd(self.Dg, t, self.dpred, True, False)
        o.mul(mask, gen, self.inpainted)                                        # inpainted buffer = mask*gen
        p, t = self._fwd(self.Dl, self.inpainted)
        o.adv(p, LSGAN, 1.0, self._loss("g_adv_local"), self.dpred)
        d2 = self._bwd(self.Dl, t, self.dpred, True, False)
        o.mul(d2, mask, self.tmp1)
        o.add(d1, self.tmp1, self.g_adv)
        o.recon("rmse", gen, ground, self._loss("rmse_global"), self.g_rec, self.lam1)        # :166
        o.add(self.g_adv, self.g_rec, self.g_adv)
        o.mul(mask, ground, self.tmp2)
        o.recon("rmse", self.inpainted, self.tmp2, self._loss("rmse_local"), self.g_rec, self.lam2)  # :167
        o.mul(self.g_rec, mask, self.tmp1)
        o.add(self.g_adv, self.tmp1, self.g_gen)
        self._bwd_G(gtok, self.g_gen)
        self._step_G(self.optG)                                                        # :172
        # ---- D step :178-200
        self.optD.zero_grad()
        for net, real, fake, tag in ((self.Dg, ground, gen, "global"), (self.Dl, self.tmp2, self.inpainted, "local")):
            if self.stacked:
                self._d_pair(net, real, fake, LSGAN, 1.0, 0.0, f"d_real_{tag}", f"d_fake_{tag}")
                continue
            p, t = self._fwd(net, real)
            o.adv(p, LSGAN, 1.0, self._loss(f"d_real_{tag}"), self.dpred)
            self._bwd(net, t, self.dpred, False, True)
            p, t = self._fwd(net, fake)
            o.adv(p, LSGAN, 0.0, self._loss(f"d_fake_{tag}"), self.dpred)
            self._bwd(net, t, self.dpred, False, True)
        self._reduce(self.Dg)
        self._reduce(self.Dl)
        self._step(self.optD)
        return self.L
