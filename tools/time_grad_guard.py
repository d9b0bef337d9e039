"""Timing of the gradient guard: global-norm clipping and the non-finite step guard between the
gradients and Adam.  All variants of a group run in ONE process, alternating, and the median of 5 timed rounds (HIP events,
after warm-up) is reported with min ... max, as tools/time_masked_controls.py does:

  * dense:    GraphedTrainStep at 4096 x 64 -- FusedAdam(net) (plain: the launches of the commit before the guard, whose
              Adam kernels are unchanged instruction for instruction), max_grad_norm = inf (guard only) and a limit that
              clips every step;
  * pair:     GraphedHierarchicalTrainStep at 4096 x (64 + 128), the same three;
  * launches: nerf_amd_grad_guard and nerf_amd_adam_step_guarded alone, beside nerf_amd_adam_step_hyper, at n = 595,844
              and 1,191,688, back to back on one stream (so at least the launch rate), with the bytes each moves.

The plain step, timed in the same process, is the yardstick: a difference inside its rounds' spread is reported as such.
lr = 0 (the weights stay where they are, every step is the same work).  Writes profiles/grad_guard_timing.json."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nerf_simple_amd import _lib                                                                     # noqa: E402
from nerf_simple_amd.optim import FusedAdam                                                          # noqa: E402
from nerf_simple_amd.training import GraphedHierarchicalTrainStep, GraphedTrainStep                  # noqa: E402
from nerf_simple_amd.utils import synthetic                                                          # noqa: E402
from nerf_simple_amd.utils.rendering import generate_rays                                            # noqa: E402
from nerf_simple_amd.utils.xyz import spherical_to_pose                                              # noqa: E402
from time_masked_controls import against, alternate, net_on                                          # noqa: E402

LIMITS = {"plain": None, "guard, max_grad_norm = inf": float("inf"), "guard, clips every step": 1e-6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--Nc", type=int, default=64)
    ap.add_argument("--Nf", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_guard_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    B, runs = args.rays, args.runs
    pose, cam = spherical_to_pose(4, -30, 0), (args.side, args.side, synthetic.focal_from_fov(args.side))
    g = torch.Generator().manual_seed(0)
    view = generate_rays(pose, cam, dev)
    rays = view[torch.randperm(view.shape[0], generator=g)[:B].to(dev)].contiguous()
    gt = torch.rand(B, 3, generator=g).to(dev)
    out = {"config": {"rays": B, "N": args.N, "Nc": args.Nc, "Nf": args.Nf, "runs": runs, "lr": 0.0,
                      "limits": {k: (None if v is None else str(v)) for k, v in LIMITS.items()},
                      "device": torch.cuda.get_device_name(dev)}}

    # ---- 1. the dense step and the pair ----
    for group in ("dense", "pair"):
        steppers = {}
        for name, limit in LIMITS.items():
            kw = dict(device_rng=True, seed=7, check_every=0)
            if group == "dense":
                net = net_on(dev)
                steppers[name] = GraphedTrainStep(net, FusedAdam(net, lr=0.0, max_grad_norm=limit), B, args.N, **kw)
            else:
                nets = [net_on(dev, seed) for seed in (1, 2)]
                steppers[name] = GraphedHierarchicalTrainStep(nets[0], nets[1], FusedAdam(nets, lr=0.0, max_grad_norm=limit), B,
                                                              args.Nc, args.Nf, **kw)
        out[group] = against(alternate({k: (lambda s=s: s.step(rays, gt)) for k, s in steppers.items()}, runs, 50, 10), "plain")
        for name, s in steppers.items():
            if s.opt.guard is not None:
                out[group][name]["record"] = s.opt.guard_stats()
        del steppers

    # ---- 2. the launches alone ----
    out["launches"] = {}
    for n in (595844, 2 * 595844):
        f32 = dict(dtype=torch.float32, device=dev)
        p, m, v = (torch.zeros(n, **f32) for _ in range(3))
        grads = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(dev)
        hyper = torch.tensor([0.0, 0.9, 0.999, 1e-8, 0.1, 0.0316, 0, 0], **f32)
        guard = torch.zeros(8, **f32)
        guard[0] = 1e-6
        ws = _lib.workspace(_lib.lib().nerf_amd_grad_guard_workspace_bytes(n), dev)
        calls = {"nerf_amd_adam_step_hyper": lambda: _lib.launch("nerf_amd_adam_step_hyper", p, grads, m, v, n, hyper, dev=dev),
                 "nerf_amd_grad_guard": lambda: _lib.launch("nerf_amd_grad_guard", grads, n, ws, guard, dev=dev),
                 "nerf_amd_adam_step_guarded": lambda: _lib.launch("nerf_amd_adam_step_guarded", p, grads, m, v, n, hyper, guard,
                                                                   dev=dev)}
        table = alternate(calls, runs, 200, 20)
        for k, t in table.items():
            t["bytes"] = 4 * n if k == "nerf_amd_grad_guard" else 7 * 4 * n          # g read; or g, p, m, v read and p, m, v written
        table["note"] = "back-to-back eager launches on one stream: at these sizes the launch rate bounds them from below"
        out["launches"][str(n)] = table

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
