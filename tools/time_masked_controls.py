"""Timing of the masked training steps with their controls: background, sigma noise and distortion loss
in the masked head.  All variants of a group run in ONE process, alternating, and the median of 5 timed rounds (HIP events,
after warm-up) is reported with min ... max, as tools/time_guided_masked.py does:

  * masked:  GraphedMaskedTrainStep at 4096 rays x 64 on the radius-1 ball with capacity = 0.25 -- plain (the step without
             ``controls=``: the kernels it had before, the baseline), background, noise, distortion, all three;
  * guided:  GraphedMaskedGuidedTrainStep at 4096 rays x (64 + 128) on the same ball with a tight capacity (largest live count
             of 8 eager steps plus a 256-row margin) -- plain and all three.

lr = 0: every replay sees the weights the live counts were measured with.  Writes profiles/masked_controls_timing.json."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_simple_amd.optim import FusedAdam                                                          # noqa: E402
from nerf_simple_amd.training import (Controls, GraphedMaskedGuidedTrainStep, GraphedMaskedTrainStep,   # noqa: E402
                                      train_step_guided)
from nerf_simple_amd.utils import synthetic                                                          # noqa: E402
from nerf_simple_amd.utils.nets import Nerf                                                          # noqa: E402
from nerf_simple_amd.utils.occupancy import OccupancyGrid                                            # noqa: E402
from nerf_simple_amd.utils.proposal import ProposalVolume                                            # noqa: E402
from nerf_simple_amd.utils.rendering import generate_rays                                            # noqa: E402
from nerf_simple_amd.utils.xyz import spherical_to_pose                                              # noqa: E402

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))


def alternate(variants, runs, reps, warmup):
    """{name: median ms per call, min, max} of callables timed in alternating order."""
    for f in variants.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for r in range(runs):
        for name in (list(variants) if r % 2 == 0 else list(variants)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                variants[name]()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in times.items()}


def net_on(dev, seed=1, kind="structured"):
    n = Nerf(precision="bf16").to(dev)
    n.load_state_dict(synthetic.synthetic_state_dict(seed, kind))
    return n


def ball_grid(R, radius, dev):
    c = (torch.arange(R - 1, dtype=torch.float64, device=dev) + 0.5) * (3.0 / (R - 1)) - 1.5
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    return OccupancyGrid.from_mask(X * X + Y * Y + Z * Z <= radius * radius, BOUNDS, outside="empty")


def against(table, baseline):
    """each variant's median beside the baseline's: the difference, and whether it lies inside the baseline's own spread"""
    b = table[baseline]
    for v in table.values():
        v["vs_plain_ms"] = round(v["median_ms"] - b["median_ms"], 4)
        v["inside_plain_spread"] = bool(b["min_ms"] <= v["median_ms"] <= b["max_ms"])
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--Nc", type=int, default=64)
    ap.add_argument("--Nf", type=int, default=128)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--capacity", type=float, default=0.25)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_controls_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    B, N, Nc, Nf, runs = args.rays, args.N, args.Nc, args.Nf, args.runs
    occ = ball_grid(args.resolution, args.radius, dev)
    g = torch.Generator().manual_seed(0)
    view = generate_rays(spherical_to_pose(4, -30, 0), (args.side, args.side, synthetic.focal_from_fov(args.side)), dev)
    rays = view[torch.randperm(view.shape[0], generator=g)[:B].to(dev)].contiguous()
    gt, bg = torch.rand(B, 3, generator=g).to(dev), torch.rand(B, 3, generator=g).to(dev)
    terms = {"plain": None, "background": Controls(background=bg), "noise": Controls(sigma_noise=1.0, noise_seed=3),
             "distortion": Controls(distortion=0.01),
             "all three": Controls(background=bg, sigma_noise=1.0, noise_seed=3, distortion=0.01)}
    out = {"config": {"rays": B, "N": N, "Nc": Nc, "Nf": Nf, "capacity": args.capacity,
                      "grid": {"resolution": args.resolution, "ball_radius": args.radius, "outside": occ.outside,
                               "cell_fraction": round(occ.cell_fraction, 4)},
                      "controls": {"sigma_noise": 1.0, "distortion": 0.01, "background": "one colour per ray"},
                      "runs": runs, "reps_per_round": 50, "device": torch.cuda.get_device_name(dev)}}

    # ---- the masked step ----
    steppers = {}
    for name, c in terms.items():
        net = net_on(dev)
        steppers[name] = GraphedMaskedTrainStep(net, FusedAdam(net, lr=0.0), B, N, occ, args.capacity, device_rng=True, seed=7,
                                                check_every=0, controls=c)
    out["masked"] = against(alternate({k: (lambda s=s: s.step(rays, gt)) for k, s in steppers.items()}, runs, 50, 10), "plain")
    for name, s in steppers.items():
        cnt = s.counts()
        out["masked"][name].update(live_last_step=cnt["live"], capacity=cnt["capacity"], overflowed=cnt["live"] > cnt["capacity"])
    del steppers

    # ---- the masked guided step ----
    prop = ProposalVolume(args.resolution, BOUNDS, device=dev).update(net_on(dev))
    probe = net_on(dev)
    opt = FusedAdam(probe, lr=0.0)
    live = 0
    for k in range(1, 9):
        train_step_guided(probe, opt, rays, gt, Nc, Nf, prop, device_rng=True, seed=7 + k, occupancy=occ)
        live = max(live, occ.last_stats["live"])
    C = min(-(-(live + 256) // 256) * 256, B * (Nc + Nf))
    steppers = {}
    for name in ("plain", "all three"):
        net = net_on(dev)
        steppers[name] = GraphedMaskedGuidedTrainStep(net, FusedAdam(net, lr=0.0), B, Nc, Nf, prop, occ, C, device_rng=True, seed=7,
                                                      check_every=0, controls=terms[name])
    out["guided"] = against(alternate({k: (lambda s=s: s.step(rays, gt)) for k, s in steppers.items()}, runs, 50, 10), "plain")
    for name, s in steppers.items():
        cnt = s.counts()
        out["guided"][name].update(live_last_step=cnt["live"], capacity=cnt["capacity"], overflowed=cnt["live"] > cnt["capacity"])
    out["guided"]["capacity_fraction"] = round(C / (B * (Nc + Nf)), 4)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
