"""Timing of the graphed coarse + fine pair with its controls: background and sigma noise in both heads.
All variants of a group run in ONE process, alternating, and the median of 5 timed rounds (HIP events, after warm-up) is reported
with min ... max and the rounds' spread, as tools/time_masked_controls.py does:

  * dense:   GraphedHierarchicalTrainStep at 4096 rays x (64 + 128) -- plain (the step without ``controls=``: the launches it had
             before, the baseline), background, noise, both;
  * masked:  GraphedMaskedHierarchicalTrainStep on the radius-1 ball, the setup of tools/time_occupancy_hierarchical.py, at the
             tight capacities profiles/occupancy_hierarchical_timing.json records for that grid -- raised, for all four variants
             alike, to the largest live count of 8 eager steps with both terms plus the 256-row margin where the noise moves the
             fine samples beyond them -- plain, background, noise, both.

lr = 0: every replay sees the weights the live counts were measured with.  Writes profiles/pair_controls_timing.json."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_simple_amd.optim import FusedAdam                                                                  # noqa: E402
from nerf_simple_amd.training import (Controls, GraphedHierarchicalTrainStep, GraphedMaskedHierarchicalTrainStep,   # noqa: E402
                                      train_step_hierarchical)
from nerf_simple_amd.utils import synthetic                                                                  # noqa: E402
from nerf_simple_amd.utils.nets import Nerf                                                                  # noqa: E402
from nerf_simple_amd.utils.occupancy import OccupancyGrid                                                    # noqa: E402
from nerf_simple_amd.utils.rendering import generate_rays                                                    # noqa: E402
from nerf_simple_amd.utils.xyz import spherical_to_pose                                                      # noqa: E402

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R = 129
REPS = 50


def alternate(variants, runs, reps, warmup):
    """{name: median ms per call, min, max, spread = (max - min) / median} of callables timed in alternating order."""
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
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "spread": round((max(v) - min(v)) / float(np.median(v)), 4)} for k, v in times.items()}


def against(table, baseline):
    """each variant's median beside the baseline's: the difference, and whether it lies inside the baseline's own spread"""
    b = table[baseline]
    for v in table.values():
        v["vs_plain_us"] = round(1000.0 * (v["median_ms"] - b["median_ms"]), 2)
        v["inside_plain_spread"] = bool(b["min_ms"] <= v["median_ms"] <= b["max_ms"])
    return table


def new_pair(dev):
    nets = []
    for seed in (0, 1):
        net = Nerf(precision="bf16").to(dev)
        net.load_state_dict(synthetic.synthetic_state_dict(seed, "structured"))
        nets.append(net)
    return nets


def ball_grid(radius, dev):
    c = (torch.arange(R - 1, dtype=torch.float64, device=dev) + 0.5) * (3.0 / (R - 1)) - 1.5
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    return OccupancyGrid.from_mask(X * X + Y * Y + Z * Z <= radius * radius, BOUNDS, outside="empty")


def up256(n, total):
    return min(-(-(n + 256) // 256) * 256, total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_controls_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    side, Nc, Nf, seed, runs = 64, 64, 128, 0, args.runs
    B, M = side * side, Nc + Nf
    rays = generate_rays(np.asarray(spherical_to_pose(4, 30, 45), dtype=np.float32), [side, side, synthetic.focal_from_fov(side)], dev)
    g = torch.Generator().manual_seed(0)
    gt, bg = torch.rand(B, 3, generator=g).to(dev), torch.rand(B, 3, generator=g).to(dev)
    terms = {"plain": None, "background": Controls(background=bg), "noise": Controls(sigma_noise=1.0, noise_seed=3),
             "both": Controls(background=bg, sigma_noise=1.0, noise_seed=3)}
    out = {"config": {"rays": B, "Nc": Nc, "Nf": Nf, "controls": {"sigma_noise": 1.0, "background": "one colour per ray"},
                      "runs": runs, "reps_per_round": REPS, "device": torch.cuda.get_device_name(dev)}}

    # ---- the dense pair ----
    steppers = {}
    for name, c in terms.items():
        nets = new_pair(dev)
        steppers[name] = GraphedHierarchicalTrainStep(*nets, FusedAdam(nets, lr=0.0), B, Nc, Nf, device_rng=True, seed=seed, check_every=0,
                                                      controls=c)
    out["dense"] = against(alternate({k: (lambda s=s: s.step(rays, gt)) for k, s in steppers.items()}, runs, REPS, 10), "plain")
    del steppers

    # ---- the masked pair on the radius-1 ball ----
    occ = ball_grid(1.0, dev)
    with open(os.path.join(ROOT, "profiles", "occupancy_hierarchical_timing.json")) as f:
        recorded = tuple(json.load(f)["grids"]["ball_1.0"]["graphed_masked"]["tight"]["capacity"])
    probe = new_pair(dev)
    opt = torch.optim.SGD([p for n in probe for p in n.parameters()], lr=0.0)
    live_c = live_f = 0
    for k in range(1, 9):
        train_step_hierarchical(*probe, opt, rays, gt, Nc, Nf, device_rng=True, seed=seed + k, occupancy=occ,
                                controls=terms["both"].replace(noise_seed=3 + k))
        live_c, live_f = max(live_c, occ.last_stats["coarse"]["live"]), max(live_f, occ.last_stats["fine"]["live"])
    cap = (max(recorded[0], up256(live_c, B * Nc)), max(recorded[1], up256(live_f, B * M)))
    steppers = {}
    for name, c in terms.items():
        nets = new_pair(dev)
        steppers[name] = GraphedMaskedHierarchicalTrainStep(*nets, FusedAdam(nets, lr=0.0), B, Nc, Nf, occ, cap, device_rng=True, seed=seed,
                                                            check_every=0, controls=c)
    out["masked"] = against(alternate({k: (lambda s=s: s.step(rays, gt)) for k, s in steppers.items()}, runs, REPS, 10), "plain")
    for name, s in steppers.items():
        cnt = s.counts()
        out["masked"][name].update(live_last_step=[cnt["coarse"]["live"], cnt["fine"]["live"]],
                                   overflowed=cnt["coarse"]["live"] > cap[0] or cnt["fine"]["live"] > cap[1])
    out["masked_config"] = {"grid": {"resolution": R, "ball_radius": 1.0, "outside": occ.outside},
                            "capacity": list(cap), "capacity_recorded_for_the_plain_pair": list(recorded),
                            "live_max_of_8_eager_steps_with_both_terms": [live_c, live_f],
                            "capacity_fraction": [round(cap[0] / (B * Nc), 4), round(cap[1] / (B * M), 4)]}

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
