"""Fused optimizers with the torch.optim call surface the plugins use:
    optim.Adam(net.parameters(), lr=0.0002, betas=(0.5, 0.999))     minimaxgan_l1.py:64-65
    optim.RMSprop(net.parameters(), lr=0.00005)                     wgan_l1.py:64-65
One kernel per network over its flat fp32 parameter / gradient / state buffers."""
import contextlib
import itertools

import torch

from . import backend as B


class _FlatOptimizer:
    def __init__(self, params):
        params = list(params)
        if not params:
            raise ValueError("optimizer got an empty parameter list")
        owners = []
        for p in params:
            owner = getattr(p, "_gi_owner", None)
            if owner is None:
                raise B.BackendError("parameter does not belong to a HIP-backend network on a gfx950 device "
                                     "(move the network with .to('cuda') before building the optimizer)")
            if all(owner is not o for o in owners):
                owners.append(owner)
        for o in owners:
            mine = sum(1 for p in params if getattr(p, "_gi_owner", None) is o)
            if mine != sum(1 for _ in o.parameters()):
                raise B.BackendError("the fused optimizers update whole networks: pass all of net.parameters()")
        self.nets = owners
        self.param_groups = [dict(params=params)]
        self.grad_scale = 1.0   # multiplies every gradient (e.g. 1/world_size after a SUM all-reduce)
        # fp16 overflow guard: scan the gradients before every update and skip the whole update when they hold
        # inf/NaN (like torch.cuda.amp.GradScaler.step). On by default for networks computing in fp16.
        self.guard = any(getattr(n, "_dtype", None) == B.GI_F16 for n in owners)
        self._flags = None
        self._seen = 0

    def _guard_ptr(self):
        """Run the finite check over the gradients of EVERY network of this optimizer into one shared verdict (all of
        them skip the update or none does, and a skipped update counts once whatever the number of networks); returns
        (device flag pointer, scan word) - (None, 0) when the guard is off. No finish launch: the update's first
        optimizer kernel records the verdict (gi_*_step_scan, include/ganinpaint.h); updates alternate between two scan words."""
        if not self.guard:
            return None, 0
        lib = B.lib()
        if self._flags is None:
            self._flags = torch.zeros(4, dtype=torch.int32, device=self.nets[0].flat_params().device)
            self._word = 3
        self._word = 5 - self._word      # 2, 3, 2, ...
        for net in self.nets:
            g = net.flat_grads()
            B.check(lib.gi_check_finite_scan_word(B.get_ctx(g.device), B.ptr(g), g.numel(), B.ptr(self._flags), self._word))
        return B.ptr(self._flags), self._word

    def poll_skipped(self):
        """Number of updates skipped since the last poll (one device read-back: call it at logging cadence)."""
        if not self.guard or self._flags is None:
            return 0
        total = int(self._flags[0].item())
        new, self._seen = total - self._seen, total
        return new

    def zero_grad(self, set_to_none=False):
        for n in self.nets:
            n.zero_grad()

    # ---- resumable training: everything an update reads besides the parameters and the gradients ----
    kind = None
    _moments = ()          # names of the per-network flat state tensors
    _hyper = ()            # attribute names of the hyper-parameters

    def _counts(self):
        """Per network [parameter count, floats of the flat buffer]: the flat buffer pads every tensor to 64 floats, so two
        networks of different shapes can share its length."""
        return [[int(sum(p.numel() for p in n.parameters())), int(n.flat_params().numel())] for n in self.nets]

    def state_dict(self):
        """CPU copy of the optimizer: per network the flat moment tensors, the hyper-parameters, and the overflow guard (its four
        device ints, the scan word of the last update, the skipped updates already polled). One device read-back."""
        guard = None
        if self._flags is not None:
            guard = dict(flags=self._flags.detach().cpu().clone(), word=int(self._word), seen=int(self._seen))
        return dict(kind=self.kind, hyper={k: getattr(self, k) for k in self._hyper},
                    counts=self._counts(),
                    state=[{k: st[k].detach().cpu().clone() for k in self._moments} for st in self.state], guard=guard)

    def load_state_dict(self, sd):
        if sd.get("kind") != self.kind:
            raise B.BackendError(f"optimizer state of kind {sd.get('kind')!r} loaded into {self.kind!r}")
        mine = self._counts()
        if [list(c) for c in sd["counts"]] != mine:
            raise B.BackendError(f"optimizer state holds networks of {[list(c) for c in sd['counts']]} [parameters, flat floats], "
                                 f"this optimizer updates {mine}")
        for i, (st, src) in enumerate(zip(self.state, sd["state"])):
            for k in self._moments:
                if k not in src or src[k].numel() != st[k].numel():
                    raise B.BackendError(f"optimizer state of network {i}: tensor {k!r} has "
                                         f"{src[k].numel() if k in src else 'no'} elements, expected {st[k].numel()}")
                st[k].copy_(src[k].to(torch.float32).view_as(st[k]))
        for k in self._hyper:
            setattr(self, k, sd["hyper"][k])
        if sd.get("guard") is None:
            self._flags, self._seen = None, 0
        else:
            g = sd["guard"]
            if g["flags"].numel() != 4:
                raise B.BackendError(f"optimizer state: the overflow guard holds {g['flags'].numel()} ints, expected 4")
            self._flags = g["flags"].to(torch.int32).to(self.nets[0].flat_params().device)
            self._word, self._seen = int(g["word"]), int(g["seen"])

    def _done(self):
        for n in self.nets:
            n.mark_dirty()


class Adam(_FlatOptimizer):
    kind, _moments, _hyper = "adam", ("m", "v"), ("lr", "betas", "eps", "t")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.state = [dict(m=torch.zeros_like(n.flat_params()), v=torch.zeros_like(n.flat_params())) for n in self.nets]
        self.t = 0

    @torch.no_grad()
    def step(self):
        self.t += 1
        lib = B.lib()
        guard, word = self._guard_ptr()
        for k, (n, st) in enumerate(zip(self.nets, self.state)):
            p, g = n.flat_params(), n.flat_grads()
            # self.t still counts the updates skipped since the last poll_skipped(); the kernel subtracts them (device count - _seen)
            B.check(lib.gi_adam_step_scan(B.get_ctx(p.device), B.ptr(p), B.ptr(g), B.ptr(st["m"]), B.ptr(st["v"]), p.numel(),
                                          self.lr, self.betas[0], self.betas[1], self.eps, self.t, self._seen if guard else -1,
                                          self.grad_scale, guard, word, 1 if k == 0 else 0))
        self._done()

    def poll_skipped(self):
        new = super().poll_skipped()
        self.t -= new     # one per skipped UPDATE (shared verdict): skipped updates do not advance the bias correction (the kernel
        #                   already left them out - device count minus _seen - so nothing changes for the updates in between)
        return new


class RMSprop(_FlatOptimizer):
    """torch.optim.RMSprop defaults (alpha=0.99, eps=1e-8, no momentum, not centered). `clamp` > 0
    fuses the WGAN weight clipping p.data.clamp_(-clamp, clamp) into the same pass."""
    kind, _moments, _hyper = "rmsprop", ("sq",), ("lr", "alpha", "eps", "clamp")

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, clamp=0.0):
        super().__init__(params)
        self.lr, self.alpha, self.eps, self.clamp = lr, alpha, eps, clamp
        self.state = [dict(sq=torch.zeros_like(n.flat_params())) for n in self.nets]

    @torch.no_grad()
    def step(self):
        lib = B.lib()
        guard, word = self._guard_ptr()
        for k, (n, st) in enumerate(zip(self.nets, self.state)):
            p, g = n.flat_params(), n.flat_grads()
            B.check(lib.gi_rmsprop_step_scan(B.get_ctx(p.device), B.ptr(p), B.ptr(g), B.ptr(st["sq"]), p.numel(), self.lr,
                                             self.alpha, self.eps, self.clamp, self.grad_scale, guard, word, 1 if k == 0 else 0))
        self._done()


class EMA:
    """Exponential moving average of a network's parameters: a flat fp32 copy of net.flat_params(), taken here, that update()
    moves towards the live parameters by (1 - decay) in one HIP pass (gi_ema_update). BatchNorm running statistics are not
    averaged: the averaged network runs with the live ones."""

    def __init__(self, net, decay):
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"EMA decay {decay!r} outside [0, 1]")
        p = net.flat_params()
        if not p.is_cuda:
            raise B.BackendError("EMA needs a network on a gfx950 device (move it with .to('cuda') first)")
        self.net, self.decay = net, float(decay)
        self.flat = p.detach().clone()

    @torch.no_grad()
    def update(self, opt=None):
        """Call right after opt.step() on the same stream. With `opt`'s overflow guard on, an update the optimizer skipped is
        skipped here as well (the verdict its first kernel recorded); no host synchronisation."""
        p = self.net.flat_params()
        guard = opt._flags if (opt is not None and opt.guard and opt._flags is not None) else None
        B.check(B.lib().gi_ema_update(B.get_ctx(p.device), B.ptr(self.flat), B.ptr(p), p.numel(), self.decay, B.ptr(guard)))

    def state_dict(self):
        return dict(decay=self.decay, flat=self.flat.detach().cpu().clone())

    def load_state_dict(self, sd):
        if sd["flat"].numel() != self.flat.numel():
            raise B.BackendError(f"EMA state holds {sd['flat'].numel()} parameters, the network has {self.flat.numel()}")
        if float(sd["decay"]) != self.decay:
            raise B.BackendError(f"EMA state was averaged with decay {sd['decay']!r}, this one uses {self.decay!r}")
        self.flat.copy_(sd["flat"].to(torch.float32).view_as(self.flat))

    @contextlib.contextmanager
    def applied(self):
        """The averaged weights in the live network for the duration of the block; the raw ones come back bit for bit. The two
        flat buffers swap contents (through one temporary copy), and the network is marked dirty both times so that its
        packed weight copies follow."""
        p = self.net.flat_params()
        with torch.no_grad():
            raw = p.detach().clone()
            p.copy_(self.flat)
            self.flat.copy_(raw)
            del raw
        self.net.mark_dirty()
        try:
            yield self.net
        finally:
            p = self.net.flat_params()
            with torch.no_grad():
                avg = p.detach().clone()
                p.copy_(self.flat)
                self.flat.copy_(avg)
                del avg
            self.net.mark_dirty()


def chain(*its):
    return itertools.chain(*its)
