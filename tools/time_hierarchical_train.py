"""Timing of the hierarchical (coarse + fine) training step, GraphedHierarchicalTrainStep at 4096 rays x (64 + 128):

  * the graphed pair step (bf16 storage, counter-RNG jitter), HIP events around runs of replays after warm-up;
  * A/B in the same process, alternating: the same step with the coarse head done as the composition
    nerf_amd_volume_render_mse_backward + nerf_amd_volume_render_rays (w to HBM) + nerf_amd_sample_pdf;

Kernel-level numbers come from a rocprofv3 run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/time_hierarchical_train.py --rounds 2
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_simple_amd import _lib                                                    # noqa: E402
from nerf_simple_amd.optim import FusedAdam                                         # noqa: E402
from nerf_simple_amd.training import GraphedHierarchicalTrainStep                  # noqa: E402
from nerf_simple_amd.utils import synthetic                                         # noqa: E402
from nerf_simple_amd.utils.nets import Nerf                                         # noqa: E402


class ComposedHead(GraphedHierarchicalTrainStep):
    """The B side: the coarse head as the three entry points it fuses (the weights make a round trip through HBM)."""

    def _alloc_pass_buffers(self, tn, tf):
        super()._alloc_pass_buffers(tn, tf)
        f32 = dict(dtype=torch.float32, device=self.dev)
        self._w = torch.empty((self.B, self.Nc), **f32)
        self._junk = [torch.empty(s_, **f32) for s_ in ((self.B, 3), (self.B,), (self.B, self.Nc), (self.B,))]

    def _coarse_head(self, c, st):
        lib, ptr, B, Nc = _lib.lib(), _lib.ptr, self.B, self.Nc
        (jit_f, ts_f, Nf), (_, _, _, flags, seed, rid) = self._pdf, c.jitter
        _lib.check(lib.nerf_amd_volume_render_mse_backward(ptr(c.raw), ptr(c.ts), ptr(self.rays), ptr(self.gt), ptr(c.rgb),
                                                           ptr(c.d_raw), B, Nc, st), "nerf_amd_volume_render_mse_backward")
        rgb, disp, alpha, acc = self._junk
        _lib.check(lib.nerf_amd_volume_render_rays(ptr(c.raw), ptr(c.ts), ptr(self.rays), ptr(rgb), ptr(disp), ptr(alpha),
                                                   ptr(acc), ptr(self._w), B, Nc, st), "nerf_amd_volume_render_rays")
        # nerf_amd_sample_pdf takes its seed as an argument only: the seed-in-memory form is the fused head's
        _lib.check(lib.nerf_amd_sample_pdf(ptr(c.ts), ptr(self._w), jit_f if not flags else None, flags & _lib.FLAG_DEVICE_RNG,
                                           seed, rid, ts_f, B, Nc, Nf, st), "nerf_amd_sample_pdf")


def make(cls, dev, B, Nc, Nf, device_rng):
    nets = []
    for s in (0, 1):
        n = Nerf(precision="bf16").to(dev)
        n.load_state_dict(synthetic.synthetic_state_dict(s, "default"))
        nets.append(n)
    opt = FusedAdam(nets, lr=5e-4)
    return cls(nets[0], nets[1], opt, B, Nc, Nf, device_rng=device_rng, seed=7, check_every=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--Nc", type=int, default=64)
    ap.add_argument("--Nf", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50, help="replays per timed run")
    ap.add_argument("--rounds", type=int, default=6, help="alternating A / B runs")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu-jitter", action="store_true", help="the reference's torch.rand stream instead of the counter RNG")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, Nc, Nf = args.rays, args.Nc, args.Nf
    g = torch.Generator().manual_seed(0)
    rays = torch.randn(B, 6, generator=g)
    rays[:, :3] *= 0.1
    rays, gt = rays.to(dev), torch.rand(B, 3, generator=g).to(dev)
    device_rng = not args.cpu_jitter
    # the counter-RNG form reads its seed from device memory; the composed B side cannot (nerf_amd_sample_pdf takes it as an
    # argument), so both sides run with explicit jitter buffers when timing the A/B: same inputs, same work
    steppers = {"fused head": make(GraphedHierarchicalTrainStep, dev, B, Nc, Nf, False),
                "composed head": make(ComposedHead, dev, B, Nc, Nf, False)}
    u_c, u_f = torch.rand(B, Nc, device=dev), torch.rand(B, Nf, device=dev)
    for s in steppers.values():
        for _ in range(args.warmup):
            s.step(rays, gt, u_c=u_c, u_f=u_f)
    torch.cuda.synchronize()
    times = {k: [] for k in steppers}
    for r in range(args.rounds):
        for name in (list(steppers) if r % 2 == 0 else list(steppers)[::-1]):
            s = steppers[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                s.step(rays, gt, u_c=u_c, u_f=u_f)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.steps)
    print(f"graphed pair step, {B} rays x ({Nc} + {Nf}), explicit jitter, {args.rounds} alternating runs of {args.steps} replays:")
    for name, ts in times.items():
        ts = sorted(ts)
        print(f"  {name:14s} median {ts[len(ts) // 2]:.4f} ms  min {ts[0]:.4f}  max {ts[-1]:.4f}")
    a, b = sorted(times["fused head"]), sorted(times["composed head"])
    print(f"  fused - composed (medians): {(a[len(a) // 2] - b[len(b) // 2]) * 1e3:+.1f} us per step")
    if device_rng:
        s = make(GraphedHierarchicalTrainStep, dev, B, Nc, Nf, True)
        for _ in range(args.warmup):
            s.step(rays, gt)
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                s.step(rays, gt)
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) / args.steps)
        runs.sort()
        print(f"graphed pair step, counter-RNG jitter (no host work): median {runs[len(runs) // 2]:.4f} ms  "
              f"min {runs[0]:.4f}  max {runs[-1]:.4f}")
        print(f"  losses after {s.opt.step_count} steps: {[round(float(x), 6) for x in s.losses]}")


if __name__ == "__main__":
    main()
