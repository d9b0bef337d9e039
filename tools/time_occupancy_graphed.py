"""Time the graphed masked training step against the dense graphed step and the eager masked step on one GPU
(profiles/occupancy_graphed_timing.json).

At 4096 rays x 64 samples, bf16, device RNG, camera spherical_to_pose(4, 30, 45) (a 64 x 64 view), t in [2, 6], structured
synthetic weights, learning rate 0 so that every step does the same work on the same weights; grids: balls of radius 1.0 /
0.75 / 0.5 in a 129^3 grid over [-1.5, 1.5]^3 with outside='empty', and the all-live grid:

  * graphed_dense   -- training.GraphedTrainStep (no grid);
  * eager_masked    -- training.train_step(..., occupancy=grid), its one host synchronisation included;
  * graphed_masked  -- training.GraphedMaskedTrainStep at the capacities {P' rounded up to 256 ("tight"), 0.25, 0.5, 1.0} B N
                       that hold the grid's live count P';
  * the two new kernels (capped emit, fused masked head) alone, through the C ABI on the stepper's own buffers;
  * from the tight capacities of the radius-1 ball and the all-live grid, the live fraction at which the graphed masked step
    and the graphed dense step cost the same.
All variants live in ONE process and are ALTERNATED round by round; a sample is the HIP-event time of `inner` back-to-back
steps after a warm-up, the reported figure the median over the rounds, and the spread (max - min over the rounds, relative
to the median) is recorded beside it.

usage: python tools/time_occupancy_graphed.py [--out profiles/occupancy_graphed_timing.json] [--rounds 9]     (GPU box)
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
from nerf_simple_amd import _lib  # noqa: E402
from nerf_simple_amd.optim import FusedAdam  # noqa: E402
from nerf_simple_amd.training import GraphedMaskedTrainStep, GraphedTrainStep, train_step  # noqa: E402
from nerf_simple_amd.utils import occupancy, synthetic  # noqa: E402
from nerf_simple_amd.utils.nets import Nerf  # noqa: E402
from nerf_simple_amd.utils.rendering import generate_rays  # noqa: E402
from nerf_simple_amd.utils.xyz import spherical_to_pose  # noqa: E402

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R = 129
FRACTIONS = (0.25, 0.5, 1.0)


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


def new_net(dev):
    net = Nerf(precision="bf16").to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, "structured"))
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy_graphed_timing.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert args.rounds >= 7, "at least 7 rounds"
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    side, N, seed = 64, 64, 0
    B = side * side
    pose = np.asarray(spherical_to_pose(4, 30, 45), dtype=np.float32)
    rays = generate_rays(pose, [side, side, synthetic.focal_from_fov(side)], dev)
    gt = torch.rand(B, 3, device=dev)
    grids = {f"ball_{r}": occupancy.OccupancyGrid.from_mask(ball_mask(r, dev), BOUNDS, outside="empty") for r in (1.0, 0.75, 0.5)}
    grids["all_live"] = occupancy.OccupancyGrid.from_mask(torch.ones((R - 1,) * 3, dtype=torch.bool, device=dev), BOUNDS)
    res = {"device": torch.cuda.get_device_name(0), "step": {"rays": B, "N": N, "samples": B * N, "precision": "bf16"},
           "grid": {"resolution": R, "bounds": BOUNDS}, "rounds": args.rounds, "inner_steps_per_sample": args.inner}

    # ---- the variants ----
    variants, meta, steppers = {}, {}, {}
    dense_net = new_net(dev)
    dense = GraphedTrainStep(dense_net, FusedAdam(dense_net, lr=0.0), B, N, device_rng=True, seed=seed, check_every=0)
    variants["graphed_dense"] = lambda: dense.step(rays, gt)
    eager_net = new_net(dev)
    eager_opt = torch.optim.SGD(eager_net.parameters(), lr=0.0)
    for name, occ in grids.items():
        # the live count of the steps that are timed: device RNG at seed + k differs from step to step, so take the largest
        # of a few steps and let the tight capacity hold it with the 256-row margin on top
        live = max(occ.mark(rays, N, device_rng=True, seed=seed + k).live for k in range(1, 9))
        tight = min(-(-(live + 256) // 256) * 256, B * N)
        meta[name] = {"outside": occ.outside, "live_samples_max_of_8_steps": live, "live_fraction": round(live / (B * N), 4)}
        variants[f"eager_masked/{name}"] = (lambda o: lambda: train_step(eager_net, eager_opt, rays, gt, N, device_rng=True,
                                                                         seed=seed + 1, occupancy=o))(occ)
        caps = {"tight": tight}
        for f in FRACTIONS:
            if int(f * B * N) > tight:
                caps[str(f)] = int(f * B * N)
        for tag, C in caps.items():
            net = new_net(dev)
            s = GraphedMaskedTrainStep(net, FusedAdam(net, lr=0.0), B, N, occ, C, device_rng=True, seed=seed, check_every=0)
            steppers[(name, tag)] = s
            variants[f"graphed_masked/{name}/{tag}"] = (lambda s_: lambda: s_.step(rays, gt))(s)
    timed = alternated(variants, args.rounds, args.inner)
    for s in steppers.values():                     # no timed step overflowed
        c = s.counts()
        assert c["live"] <= c["capacity"], c
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
            t["capacity"] = s.capacity
            t["capacity_fraction"] = round(s.capacity / (B * N), 4)
            t["over_graphed_dense"] = round(t["median_ms"] / T_dense, 4)
            t["over_eager_masked"] = round(t["median_ms"] / row["eager_masked"]["median_ms"], 4)
            row["graphed_masked"][tag] = t
        res["grids"][name] = row
        print(json.dumps({name: {k: (v if k != "graphed_masked" else {t: x["median_ms"] for t, x in v.items()})
                                 for k, v in row.items() if k != "eager_masked"}, "eager_masked_ms": row["eager_masked"]["median_ms"],
                          "graphed_dense_ms": T_dense}), flush=True)

    # ---- the claim: radius-1 ball, C = 0.25 B N ----
    ball = res["grids"]["ball_1.0"]
    if "0.25" in ball["graphed_masked"]:
        t = ball["graphed_masked"]["0.25"]
        res["claim_ball_1.0_capacity_0.25"] = {
            "graphed_masked_ms": t["median_ms"], "graphed_dense_ms": T_dense, "eager_masked_ms": ball["eager_masked"]["median_ms"],
            "graphed_masked_over_graphed_dense": t["over_graphed_dense"], "graphed_masked_over_eager_masked": t["over_eager_masked"],
            "faster_than_both": bool(t["median_ms"] < T_dense and t["median_ms"] < ball["eager_masked"]["median_ms"])}
    # break-even against the dense graph: the tight capacities of the radius-1 ball and the all-live grid, linear in between
    a, b = ball["graphed_masked"]["tight"], res["grids"]["all_live"]["graphed_masked"]["tight"]
    slope = (b["median_ms"] - a["median_ms"]) / (b["capacity_fraction"] - a["capacity_fraction"])
    fixed = a["median_ms"] - slope * a["capacity_fraction"]
    res["graphed_masked_ms_per_unit_capacity_fraction"] = round(slope, 4)
    res["graphed_masked_fixed_ms"] = round(fixed, 4)
    res["break_even_capacity_fraction"] = round((T_dense - fixed) / slope, 4) if slope > 0 else None
    res["break_even_live_fraction_note"] = ("the step's cost follows its capacity; with a tight capacity (P' + 256 rounded up to "
                                            "256) the break-even live fraction is the break-even capacity fraction less 512 / (B N)")
    res["break_even_live_fraction"] = (round(res["break_even_capacity_fraction"] - 512 / (B * N), 4)
                                       if res["break_even_capacity_fraction"] is not None else None)

    # ---- the two new kernels alone (the stepper's buffers; ball_1.0 at every capacity, all_live tight) ----
    st = _lib.stream_ptr(dev)
    res["kernels"] = {}
    for (name, tag), s in steppers.items():
        if name not in ("ball_1.0", "all_live"):
            continue
        off = torch.tensor([1], dtype=torch.int64, device=dev)
        head = (_lib.ptr(s.rays), _lib.ptr(off), _lib.ptr(s.tbins))
        flags = _lib.FLAG_DEVICE_RNG | _lib.FLAG_SEED_IN_MEMORY
        tail = (_lib.ptr(s.mask), _lib.ptr(s.offsets))
        kern = {
            "capped_emit": lambda: lib.nerf_amd_occupancy_points_capped(*head, flags, seed, 0, *tail, _lib.ptr(s.pts), _lib.ptr(s._counts),
                                                                        s.capacity, B, N, st),
            "fused_masked_head": lambda: lib.nerf_amd_volume_render_masked_mse_backward(
                _lib.ptr(s.raw), *head, flags, seed, 0, *tail, _lib.ptr(s.gt), _lib.ptr(s.rgb), _lib.ptr(s.d_raw), s.capacity, B, N, st),
        }
        k = alternated(kern, args.rounds, 10)
        res["kernels"][f"{name}/{tag}"] = {"capacity": s.capacity, **{n: {"median_ms": v["median_ms"], "spread": v["spread"]}
                                                                       for n, v in k.items()}}
    res["largest_spread"] = max(v["spread"] for v in timed.values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k.startswith(("claim", "break_even", "graphed_masked_", "largest"))}))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
