"""Timing of the scene box on the radius-1 ball with a 128^3 grid and the lego camera (distance 4,
tn = 2, tf = 6), with no box, the grid's own bounds (``SceneBox.from_grid``) and the live cells' box
(``SceneBox.from_occupancy``).  All variants of a group run in ONE process, alternating, and the median of 5 timed rounds (HIP
events, after warm-up) is reported with min ... max, as tools/time_masked_controls.py does:

  * placement:  nerf_amd_box_positions alone at 640,000 x 128 and 4096 x 64, beside the time its bytes (24 B + 4 N B per ray)
                take at the HBM rate tools/time_input_grad.py quotes (6 TB/s);
  * view:       render_view at 800 x 800 x 128, fp16, through the grid: ms, live samples, live samples per hit ray;
  * masked:     GraphedMaskedTrainStep against GraphedMaskedBoxTrainStep at 4096 x 64 -- at equal capacity, and at (about)
                equal live samples per hit ray by lowering N under the box;
  * dense:      GraphedTrainStep against GraphedBoxTrainStep: the extra node against the plain step's spread.

The step without a box, timed in the same process, is the baseline; a difference inside its rounds' spread is reported as not
resolvable.  lr = 0.  The live counts are counts, not quality: no trained scene is involved.  Writes profiles/box_timing.json."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nerf_simple_amd import _lib                                                                     # noqa: E402
from nerf_simple_amd.optim import FusedAdam                                                          # noqa: E402
from nerf_simple_amd.training import (GraphedBoxTrainStep, GraphedMaskedBoxTrainStep, GraphedMaskedTrainStep,   # noqa: E402
                                      GraphedTrainStep)
from nerf_simple_amd.utils import synthetic                                                          # noqa: E402
from nerf_simple_amd.utils.box import SceneBox                                                       # noqa: E402
from nerf_simple_amd.utils.rendering import generate_rays, render_view                               # noqa: E402
from nerf_simple_amd.utils.xyz import spherical_to_pose                                              # noqa: E402
from time_masked_controls import BOUNDS, alternate, ball_grid, net_on                                # noqa: E402

HBM_BYTES_PER_S = 6e12


def against(table, baseline):
    """each variant's median beside the baseline's: the difference, and whether it is resolvable against the baseline's spread"""
    b = table[baseline]
    for v in table.values():
        v["vs_" + baseline.replace(" ", "_") + "_ms"] = round(v["median_ms"] - b["median_ms"], 4)
        v["resolvable"] = not (b["min_ms"] <= v["median_ms"] <= b["max_ms"])
    return table


def hit_stats(box, occ, rays, N, seed):
    """(live samples, hit rays, live per hit ray) of one batch; without a box every ray counts as a hit ray"""
    if box is None:
        m = occ.mark(rays, N, device_rng=True, seed=seed)
        hits = rays.shape[0]
    else:
        ts, _, hit = box.positions(rays, N, device_rng=True, seed=seed, return_span=True)
        m = occ.mark(rays, N, ts=ts)
        hits = int(hit.sum())
    return {"live": m.live, "hit_rays": hits, "live_per_hit_ray": round(m.live / max(1, hits), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--view-N", type=int, default=128)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    B, N, runs = args.rays, args.N, args.runs
    occ = ball_grid(args.resolution, args.radius, dev)
    boxes = {"no box": None, "grid bounds": SceneBox.from_grid(occ), "live cells": SceneBox.from_occupancy(occ)}
    pose, cam = spherical_to_pose(4, -30, 0), (args.side, args.side, synthetic.focal_from_fov(args.side))
    g = torch.Generator().manual_seed(0)
    view = generate_rays(pose, cam, dev)
    rays = view[torch.randperm(view.shape[0], generator=g)[:B].to(dev)].contiguous()
    gt = torch.rand(B, 3, generator=g).to(dev)
    out = {"config": {"rays": B, "N": N, "view": [args.side, args.side, args.view_N], "tn": 2, "tf": 6,
                      "grid": {"resolution": args.resolution, "ball_radius": args.radius, "outside": occ.outside,
                               "cell_fraction": round(occ.cell_fraction, 4)},
                      "boxes": {k: None if b is None else {"lo": b.lo, "hi": b.hi} for k, b in boxes.items()},
                      "runs": runs, "device": torch.cuda.get_device_name(dev), "hbm_bytes_per_s": HBM_BYTES_PER_S}}

    # ---- 1. the placement kernel alone ----
    out["placement"] = {}
    tight = boxes["live cells"]
    for r, n, reps in ((view, args.view_N, 20), (rays, N, 200)):
        rows = r.shape[0]
        ts = torch.empty((rows, n), dtype=torch.float32, device=dev)
        u = torch.rand((rows, n), dtype=torch.float32, device=dev)
        tb01 = torch.linspace(0, 1, n + 1).to(dev)
        box_args = (_lib.host_f32x3(tight.lo), _lib.host_f32x3(tight.hi), 2.0, 6.0, _lib.ptr(ts), None, None, rows, n, _lib.stream_ptr(dev))
        # the three sources of the unit positions: ten Philox rounds per sample, or 4 N more bytes per ray read
        calls = {"counter RNG": (_lib.ptr(r), None, _lib.ptr(tb01), _lib.FLAG_DEVICE_RNG, 3, 0, *box_args),
                 "explicit u": (_lib.ptr(r), _lib.ptr(u), _lib.ptr(tb01), 0, 0, 0, *box_args),
                 "given unit positions": (_lib.ptr(r), _lib.ptr(u), None, _lib.FLAG_TS_GIVEN, 0, 0, *box_args)}
        table = alternate({k: (lambda c=c: _lib.check(_lib.lib().nerf_amd_box_positions(*c), "nerf_amd_box_positions"))
                           for k, c in calls.items()}, runs, reps, 5)
        for k, t in table.items():
            nbytes = rows * (24 + 4 * n + (0 if k == "counter RNG" else 4 * n))
            t.update(bytes=nbytes, byte_time_us=round(nbytes / HBM_BYTES_PER_S * 1e6, 2),
                     achieved_bytes_per_s=round(nbytes / (t["median_ms"] * 1e-3), -9))
        table["note"] = "back-to-back eager launches into one preallocated buffer: at the small size this is the launch rate"
        out["placement"][f"{rows} x {n}"] = table

    # ---- 2. render_view through the grid ----
    vnet = net_on(dev)
    with torch.no_grad():
        variants = {k: (lambda b=b: render_view(vnet, pose, cam, N=args.view_N, device_rng=True, seed=5, occupancy=occ, precision="fp16",
                                                **({} if b is None else {"box": b}))) for k, b in boxes.items()}
        # under the tight box: the N that gives about the plain view's live samples per hit ray
        base, boxed = hit_stats(None, occ, view, args.view_N, 5), hit_stats(tight, occ, view, args.view_N, 5)
        vn_low = max(8, int(round(args.view_N * base["live"] / max(1, boxed["live"]) / 8)) * 8)
        low = f"live cells, N = {vn_low}"
        variants[low] = lambda: render_view(vnet, pose, cam, N=vn_low, device_rng=True, seed=5, occupancy=occ, precision="fp16",
                                            box=tight)
        out["view"] = against(alternate(variants, runs, 3, 2), "no box")
        for k, b in boxes.items():
            out["view"][k].update(N=args.view_N, **hit_stats(b, occ, view, args.view_N, 5))
        out["view"][low].update(N=vn_low, **hit_stats(tight, occ, view, vn_low, 5))

    # ---- 3. the masked step ----
    stats = {k: hit_stats(b, occ, rays, N, 8) for k, b in boxes.items()}
    cap = min(-(-int(1.25 * max(s["live"] for s in stats.values())) // 256) * 256, B * N)
    # under the tight box: the N that gives about the plain step's live samples per hit ray
    ratio = stats["no box"]["live"] / max(1, stats["live cells"]["hit_rays"]) / max(1e-9, stats["live cells"]["live_per_hit_ray"])
    n_low = max(8, int(round(N * ratio / 8)) * 8)
    steppers = {}
    for k, b in boxes.items():
        net = net_on(dev)
        opt = FusedAdam(net, lr=0.0)
        kw = dict(device_rng=True, seed=7, check_every=0)
        steppers[k] = (GraphedMaskedTrainStep(net, opt, B, N, occ, cap, **kw) if b is None else
                       GraphedMaskedBoxTrainStep(net, opt, B, N, b, occ, cap, **kw))
    net = net_on(dev)
    cap_low = min(-(-int(1.25 * hit_stats(tight, occ, rays, n_low, 8)["live"]) // 256) * 256, B * n_low)
    steppers[f"live cells, N = {n_low}"] = GraphedMaskedBoxTrainStep(net, FusedAdam(net, lr=0.0), B, n_low, tight, occ, cap_low,
                                                                    device_rng=True, seed=7, check_every=0)
    out["masked"] = against(alternate({k: (lambda s=s: s.step(rays, gt)) for k, s in steppers.items()}, runs, 50, 10), "no box")
    for k, s in steppers.items():
        cnt = s.counts()
        out["masked"][k].update(N=s.N, live_last_step=cnt["live"], capacity=cnt["capacity"], overflowed=cnt["live"] > cnt["capacity"])
    for k, b in boxes.items():
        out["masked"][k].update(batch=stats[k])
    out["masked"][f"live cells, N = {n_low}"].update(batch=hit_stats(tight, occ, rays, n_low, 8))
    del steppers

    # ---- 4. the dense step: what the extra node costs ----
    steppers = {}
    for k, b in (("no box", None), ("live cells", tight)):
        net = net_on(dev)
        opt = FusedAdam(net, lr=0.0)
        kw = dict(device_rng=True, seed=7, check_every=0)
        steppers[k] = GraphedTrainStep(net, opt, B, N, **kw) if b is None else GraphedBoxTrainStep(net, opt, B, N, b, **kw)
    out["dense"] = against(alternate({k: (lambda s=s: s.step(rays, gt)) for k, s in steppers.items()}, runs, 50, 10), "no box")

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
