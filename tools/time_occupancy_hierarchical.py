"""Time the masked hierarchical pair step against the dense graphed pair step on one GPU
(profiles/occupancy_hierarchical_timing.json), in the manner of tools/time_occupancy_graphed.py.

At 4096 rays x (64 + 128) samples, bf16, device RNG, camera spherical_to_pose(4, 30, 45) (a 64 x 64 view), t in [2, 6],
structured synthetic weights (coarse: seed 0, fine: seed 1), learning rate 0 so that every step does the same work on the same
weights; grids: balls of radius 1.0 / 0.75 / 0.5 in a 129^3 grid over [-1.5, 1.5]^3 with outside='empty', and the all-live grid:

  * graphed_dense   -- training.GraphedHierarchicalTrainStep (no grid);
  * eager_masked    -- training.train_step_hierarchical(..., occupancy=grid), its two host synchronisations included;
  * graphed_masked  -- training.GraphedMaskedHierarchicalTrainStep at a tight capacity per pass (largest count observed over a
                       few steps + 256, rounded up to 256) and at 0.25 and 0.5 of each pass where those hold both counts
                       (a capacity that would overflow is not timed; it is listed under "skipped").
Beside the times: THE LIVE FRACTION OF EACH PASS.  The fine samples gather where the coarse weights are, so the fine pass's
live fraction is not the coarse pass's, and the fine capacity a user needs follows it.
All variants live in ONE process and are ALTERNATED round by round; a sample is the HIP-event time of `inner` back-to-back
steps after a warm-up, the reported figure the median over the rounds, and the spread (max - min over the rounds, relative
to the median) is recorded beside it.

usage: python tools/time_occupancy_hierarchical.py [--out profiles/occupancy_hierarchical_timing.json] [--rounds 9]   (GPU box)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nerf_simple_amd  # noqa: E402,F401
from nerf_simple_amd.optim import FusedAdam  # noqa: E402
from nerf_simple_amd.training import (GraphedHierarchicalTrainStep, GraphedMaskedHierarchicalTrainStep,  # noqa: E402
                                      train_step_hierarchical)
from nerf_simple_amd.utils import occupancy, synthetic  # noqa: E402
from nerf_simple_amd.utils.nets import Nerf  # noqa: E402
from nerf_simple_amd.utils.rendering import generate_rays  # noqa: E402
from nerf_simple_amd.utils.xyz import spherical_to_pose  # noqa: E402

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R = 129
FRACTIONS = (0.25, 0.5)


def ball_mask(radius, dev):
    c = (torch.arange(R - 1, dtype=torch.float64, device=dev) + 0.5) * (3.0 / (R - 1)) - 1.5
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    return X * X + Y * Y + Z * Z <= radius * radius


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternated(variants, rounds, inner):
    for _ in range(3):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            samples[k].append(event_ms(fn, inner))
    out = {}
    for k, v in samples.items():
        med = statistics.median(v)
        out[k] = {"median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4), "samples_ms": [round(x, 4) for x in v]}
    return out


def new_pair(dev):
    nets = []
    for seed in (0, 1):
        net = Nerf(precision="bf16").to(dev)
        net.load_state_dict(synthetic.synthetic_state_dict(seed, "structured"))
        nets.append(net)
    return nets


def up256(n, total):
    return min(-(-(n + 256) // 256) * 256, total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy_hierarchical_timing.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    assert args.rounds >= 7, "at least 7 rounds"
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    side, Nc, Nf, seed = 64, 64, 128, 0
    B, M = side * side, Nc + Nf
    pose = np.asarray(spherical_to_pose(4, 30, 45), dtype=np.float32)
    rays = generate_rays(pose, [side, side, synthetic.focal_from_fov(side)], dev)
    gt = torch.rand(B, 3, device=dev)
    grids = {f"ball_{r}": occupancy.OccupancyGrid.from_mask(ball_mask(r, dev), BOUNDS, outside="empty") for r in (1.0, 0.75, 0.5)}
    grids["all_live"] = occupancy.OccupancyGrid.from_mask(torch.ones((R - 1,) * 3, dtype=torch.bool, device=dev), BOUNDS)
    res = {"device": torch.cuda.get_device_name(0),
           "step": {"rays": B, "Nc": Nc, "Nf": Nf, "samples": [B * Nc, B * M], "precision": "bf16"},
           "grid": {"resolution": R, "bounds": BOUNDS}, "rounds": args.rounds, "inner_steps_per_sample": args.inner}

    variants, meta, steppers = {}, {}, {}
    dense_pair = new_pair(dev)
    dense = GraphedHierarchicalTrainStep(*dense_pair, FusedAdam(dense_pair, lr=0.0), B, Nc, Nf, device_rng=True, seed=seed, check_every=0)
    variants["graphed_dense"] = lambda: dense.step(rays, gt)
    eager_pair = new_pair(dev)
    eager_opt = torch.optim.SGD([p for n in eager_pair for p in n.parameters()], lr=0.0)

    def eager(occ, k=1):
        return train_step_hierarchical(*eager_pair, eager_opt, rays, gt, Nc, Nf, device_rng=True, seed=seed + k, occupancy=occ)

    for name, occ in grids.items():
        # the live counts of the steps that are timed: device RNG at seed + k differs from step to step, so take the largest of
        # a few eager steps (lr = 0: the weights, hence the sampler's weights, stay) and put the 256-row margin on top
        live_c, live_f = 0, 0
        for k in range(1, 9):
            eager(occ, k)
            live_c, live_f = max(live_c, occ.last_stats["coarse"]["live"]), max(live_f, occ.last_stats["fine"]["live"])
        tight = (up256(live_c, B * Nc), up256(live_f, B * M))
        meta[name] = {"outside": occ.outside, "live_samples_max_of_8_steps": {"coarse": live_c, "fine": live_f},
                      "live_fraction": {"coarse": round(live_c / (B * Nc), 4), "fine": round(live_f / (B * M), 4)},
                      "skipped": []}
        variants[f"eager_masked/{name}"] = (lambda o: lambda: eager(o))(occ)
        caps = {"tight": tight}
        for f in FRACTIONS:
            c = (int(f * B * Nc), int(f * B * M))
            if c[0] >= tight[0] and c[1] >= tight[1]:
                caps[str(f)] = c
            else:
                meta[name]["skipped"].append({"capacity_fraction": f, "reason": "would overflow: below the tight capacity of a pass"})
        for tag, C in caps.items():
            pair = new_pair(dev)
            s = GraphedMaskedHierarchicalTrainStep(*pair, FusedAdam(pair, lr=0.0), B, Nc, Nf, occ, C, device_rng=True, seed=seed,
                                                   check_every=0)
            steppers[(name, tag)] = s
            variants[f"graphed_masked/{name}/{tag}"] = (lambda s_: lambda: s_.step(rays, gt))(s)
    timed = alternated(variants, args.rounds, args.inner)
    for s in steppers.values():                     # no timed step overflowed
        c = s.counts()
        assert c["coarse"]["live"] <= c["coarse"]["capacity"] and c["fine"]["live"] <= c["fine"]["capacity"], c
    res["graphed_dense"] = timed["graphed_dense"]
    res["grids"] = {}
    T_dense = timed["graphed_dense"]["median_ms"]
    for name in grids:
        row = dict(meta[name])
        row["eager_masked"] = timed[f"eager_masked/{name}"]
        row["graphed_masked"] = {}
        for (g, tag), s in steppers.items():
            if g != name:
                continue
            t = dict(timed[f"graphed_masked/{name}/{tag}"])
            t["capacity"] = list(s.capacity)
            t["capacity_fraction"] = [round(s.capacity[0] / (B * Nc), 4), round(s.capacity[1] / (B * M), 4)]
            t["capacity_points_over_dense_points"] = round(sum(s.capacity) / (B * (Nc + M)), 4)
            t["over_graphed_dense"] = round(t["median_ms"] / T_dense, 4)
            t["over_eager_masked"] = round(t["median_ms"] / row["eager_masked"]["median_ms"], 4)
            row["graphed_masked"][tag] = t
        res["grids"][name] = row
        print(json.dumps({name: {"live_fraction": row["live_fraction"], "graphed_masked_ms": {t: x["median_ms"] for t, x in
                                                                                              row["graphed_masked"].items()},
                                 "eager_masked_ms": row["eager_masked"]["median_ms"], "graphed_dense_ms": T_dense}}), flush=True)
    # cost against points: the tight capacities of the radius-0.5 ball and the all-live grid, linear in between
    a, b = res["grids"]["ball_0.5"]["graphed_masked"]["tight"], res["grids"]["all_live"]["graphed_masked"]["tight"]
    dx = b["capacity_points_over_dense_points"] - a["capacity_points_over_dense_points"]
    if dx > 0:
        slope = (b["median_ms"] - a["median_ms"]) / dx
        fixed = a["median_ms"] - slope * a["capacity_points_over_dense_points"]
        res["graphed_masked_ms_per_unit_point_fraction"] = round(slope, 4)
        res["graphed_masked_fixed_ms"] = round(fixed, 4)
        res["break_even_point_fraction"] = round((T_dense - fixed) / slope, 4) if slope > 0 else None
    res["largest_spread"] = max(v["spread"] for v in timed.values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k.startswith(("break_even", "graphed_masked_", "largest"))}))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
