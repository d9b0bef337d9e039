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
"""
import torch

from . import _lib


class FusedAdam:
    nets = None

    def __init__(self, net, lr=5e-4, betas=(0.9, 0.999), eps=1e-8):
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
        _lib.launch("nerf_amd_adam_step", self.flat, g, self.exp_avg, self.exp_avg_sq, self.flat.numel(), float(pg["lr"]),
                    float(pg["betas"][0]), float(pg["betas"][1]), float(pg["eps"]), self.step_count, dev=self.flat.device)
        # the kernel wrote through the flat buffer (the parameters' _version did not move):
        # re-derive the packed images now and stamp the cache with the current versions
        if self.nets is None:
            self.net.repack_from_flat(self.flat)
        else:
            for m, sl in zip(self.nets, self.slices):
                m.repack_from_flat(sl)
