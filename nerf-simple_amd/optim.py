"""Fused optimizer for the training loop.

``FusedAdam(net)`` is the reference's ``torch.optim.Adam(net.parameters(), lr=5e-4)``
(train.py:43) with the same update rule and defaults, restructured for the GPU:

  * the 24 parameter tensors become views of ONE flat fp32 buffer (state_dict
    order), and so do the moments; ``step()`` is one HIP kernel over 595,844
    elements instead of a multi-tensor sweep;
  * ``step()`` ends by re-deriving the packed MFMA weight images the fused kernels
    stream (forward bf16 image, backward image) straight from the flat buffer;
  * ``param_groups[0]['lr']`` is honoured every step, so the reference's
    ``for p in optimizer.param_groups: p['lr'] *= decay`` loop (train.py:56-57) works
    unchanged.

``FusedAdam([net_c, net_f])`` (the hierarchical pair, training.train_step_hierarchical): the modules'
parameters, in the order given and state_dict order within each, share ONE flat vector (2 x 595,844
elements), so one Adam launch updates both; each module's packed images are then re-derived from its
own slice.  ``nets`` is that tuple (None for a single module) and ``slices`` their views of ``flat``.

``FusedAdam(net, max_grad_norm=x)``: global-norm gradient clipping and a non-finite step guard, both
decided in device memory between the gradients and the update (nerf_amd_grad_guard, nerf_amd_adam_step_guarded; the
definition is in include/nerf_amd.h).  ``x`` is a float > 0 -- ``float('inf')`` never clips and only guards -- and the norm
is ONE norm over the optimiser's whole flat gradient (both networks of a pair, as ``clip_grad_norm_`` over all parameters
gives).  A step whose norm is not finite (a NaN / inf gradient element, or a norm beyond fp32) is WITHHELD: parameters, both
moments and the packed images keep their bits.  Time still passes: ``step_count`` counts attempted steps and the bias
corrections stay those of the attempted step t, so after k skips they are those of step t, not t - k (a relative difference
of beta^(t-k) - beta^t: nothing beyond the first few hundred steps).  ``guard`` is the record (8 words, float32 view:
max_norm, norm, coef, then as int32 skip / steps / skipped / clipped / 0), ``grad_norm`` a 0-d device view of the last
step's pre-clip norm (no sync), ``set_max_grad_norm(x)`` rewrites the limit in place (captured graphs read it at every
replay), ``guard_stats()`` reads the record (one host read).  ``None`` (the default) launches exactly what it always did.
"""
import math

import torch

from . import _lib


def check_max_grad_norm(x):
    """``max_grad_norm`` as a float: a number > 0, ``float('inf')`` included; NaN, 0, a negative number or a non-number is a
    ValueError."""
    import numbers
    if isinstance(x, bool) or not isinstance(x, numbers.Real) or not float(x) > 0.0:
        raise ValueError(f"max_grad_norm must be a number > 0 (float('inf') = guard only) or None, got {x!r}")
    return float(x)


def _f32(x):
    """``x`` rounded to fp32, as a Python float (what a C ``float`` argument holds)."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def adam_scalars(lr, betas, eps, t):
    """The six scalars of Adam's step ``t`` (1-based) as every Adam kernel of the library takes them -- {lr, beta1, beta2, eps,
    1 - beta1^t, sqrt(1 - beta2^t)} -- by the rule of nerf_amd_adam_step (include/nerf_amd.h), which is the definition: the
    betas are the fp32 values the kernel multiplies by, and the two bias corrections are formed in double FROM THOSE rounded
    betas (``math.sqrt``, as the C ``sqrt``), so the update is Adam's for exactly the betas the kernel holds.  Python floats;
    storing them as fp32 is the one rounding left.  The ONE place this formula lives on the Python side: the guarded eager
    step, the graphed steppers and the per-image tables' optimiser all call it."""
    b1, b2, t = _f32(betas[0]), _f32(betas[1]), int(t)
    if t < 1:
        raise ValueError(f"Adam's step count is 1-based, got {t}")
    return (float(lr), b1, b2, float(eps), 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t))


class FusedAdam:
    nets = None
    guard = None                 # the guard record on the device (max_grad_norm given), else None
    max_grad_norm = None

    def __init__(self, net, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
        if max_grad_norm is not None:
            max_grad_norm = check_max_grad_norm(max_grad_norm)       # before the device is looked at
        if isinstance(net, (list, tuple)):
            nets = tuple(net)
            if not nets or len({id(n) for n in nets}) != len(nets):
                raise ValueError("FusedAdam([...]) takes distinct modules (the same module twice would be updated twice)")
            self.nets = nets
        self.net = net if self.nets is None else self.nets
        mods = (net,) if self.nets is None else self.nets
        self.params = [p for m in mods for _, p in m.named_parameters()]
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("FusedAdam needs the module on the GPU")
        with torch.no_grad():
            self.flat = torch.cat([p.detach().reshape(-1).float() for p in self.params]).contiguous()
            off = 0
            for p in self.params:                      # parameters become views of the flat buffer
                n = p.numel()
                p.data = self.flat[off:off + n].view(p.shape)
                off += n
        if self.nets is not None:
            self.slices, off = [], 0
            for m in mods:
                k = sum(p.numel() for p in m.parameters())
                self.slices.append(self.flat[off:off + k])
                off += k
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.param_groups = [{"params": self.params, "lr": lr, "betas": betas, "eps": eps}]
        self.step_count = 0
        self._grad = torch.empty_like(self.flat)
        if max_grad_norm is not None:
            # allocated here, before any capture: the record (word 0 = the limit), the reduction's workspace, and the device
            # vector of the eager step's six scalars (a graphed stepper feeds its own)
            self.max_grad_norm = max_grad_norm
            self.guard = torch.zeros(8, dtype=torch.float32, device=dev)
            self.guard[0] = max_grad_norm
            self._guard_ws = _lib.workspace(_lib.lib().nerf_amd_grad_guard_workspace_bytes(self.flat.numel()), dev)
            self._hyper = torch.zeros(8, dtype=torch.float32, device=dev)

    @property
    def grad_norm(self):
        """The last step's gradient norm before clipping (NaN / inf on a withheld step): a 0-d device view of the record,
        no sync.  None without ``max_grad_norm``."""
        return None if self.guard is None else self.guard[1]

    def set_max_grad_norm(self, x):
        """A new limit, written into the record in place: the next step -- eager or a replay of a captured graph -- reads it."""
        if self.guard is None:
            raise RuntimeError("this FusedAdam was built without max_grad_norm: there is no guard to set a limit on "
                               "(build it with max_grad_norm=float('inf') to guard without clipping)")
        self.max_grad_norm = check_max_grad_norm(x)
        self.guard[0:1].fill_(self.max_grad_norm)

    def guard_stats(self):
        """The record, read now (one host read, synchronises): the last step's ``norm`` and ``coef``, whether it was withheld
        (``skipped_last``), and the running totals ``steps`` / ``skipped`` / ``clipped``.  None without ``max_grad_norm``."""
        if self.guard is None:
            return None
        h = self.guard.cpu()
        w = h.view(torch.int32)
        return {"norm": float(h[1]), "coef": float(h[2]), "skipped_last": bool(w[3]), "steps": int(w[4]), "skipped": int(w[5]),
                "clipped": int(w[6])}

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def _flat_grad(self):
        # the fused backward hands out views of ONE flat vector: use it in place
        from .parallel import flat_grad_view
        flat = flat_grad_view(self.params)
        if flat is not None and flat.numel() == self.flat.numel():
            return flat
        torch.cat([p.grad.reshape(-1).float() for p in self.params], out=self._grad)
        return self._grad

    @torch.no_grad()
    def step(self):
        g = self._flat_grad()
        pg = self.param_groups[0]
        self.step_count += 1
        if self.guard is None:
            _lib.launch("nerf_amd_adam_step", self.flat, g, self.exp_avg, self.exp_avg_sq, self.flat.numel(), float(pg["lr"]),
                        float(pg["betas"][0]), float(pg["betas"][1]), float(pg["eps"]), self.step_count, dev=self.flat.device)
        else:
            # the six scalars nerf_amd_adam_step forms from its arguments, in device memory: with max_grad_norm = inf and a
            # finite gradient this step IS the plain one, bit for bit
            n, dev = self.flat.numel(), self.flat.device
            self._hyper[:6] = torch.tensor(adam_scalars(pg["lr"], pg["betas"], pg["eps"], self.step_count), dtype=torch.float32)
            _lib.launch("nerf_amd_grad_guard", g, n, self._guard_ws, self.guard, dev=dev)
            _lib.launch("nerf_amd_adam_step_guarded", self.flat, g, self.exp_avg, self.exp_avg_sq, n, self._hyper, self.guard,
                        dev=dev)
        # the kernel wrote through the flat buffer (the parameters' _version did not move):
        # re-derive the packed images now and stamp the cache with the current versions
        if self.nets is None:
            self.net.repack_from_flat(self.flat)
        else:
            for m, sl in zip(self.nets, self.slices):
                m.repack_from_flat(sl)
