"""Time the masked render (occupancy grid) against the dense render on one GPU (profiles/occupancy_timing.json).

At 800 x 800 x 128, camera spherical_to_pose(4, 30, 45), t in [2, 6], device RNG, structured synthetic weights, fp16 and
bf16; grids: balls of radius 1.0 / 0.75 / 0.5 in a 129^3 grid over [-1.5, 1.5]^3 with outside='empty', and the all-live grid:

  * T_full    -- render_view without occupancy (the dense fused render), same process;
  * T_masked  -- render_view(..., occupancy=grid) end to end, its one host synchronisation included;
  * stages    -- mark + scan, emit, the network on the P' live points (= T_pts(P'), nerf_amd_mlp_forward alone: the floor the
                 feature can reach), the masked composite, each through the C ABI on preallocated buffers, with the bytes
                 each moves at least; and the device-to-host read of the live count on an idle stream (the sync);
  * from the all-live grid and the radius-1 ball, the live fraction at which masked and dense cost the same.
HIP events around back-to-back calls after a warm-up; the variants are ALTERNATED round by round (as tools/ab_bench.py
does) and the median over the rounds is reported.

usage: python tools/time_occupancy.py [--out profiles/occupancy_timing.json] [--rounds 7] [--side 800]     (GPU box)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nerf_simple_amd  # noqa: E402,F401
from nerf_simple_amd import _lib  # noqa: E402
from nerf_simple_amd.utils import occupancy, synthetic  # noqa: E402
from nerf_simple_amd.utils.nets import Nerf  # noqa: E402
from nerf_simple_amd.utils.rendering import _tbins, generate_rays, render_view  # noqa: E402
from nerf_simple_amd.utils.xyz import spherical_to_pose  # noqa: E402

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R = 129


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


def alternated(variants, rounds, inner=2):
    """{name: median ms per call}: one warm-up pass, then `rounds` passes over all variants in turn"""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            samples[k].append(event_ms(fn, inner))
    return {k: statistics.median(v) for k, v in samples.items()}, {k: [round(x, 3) for x in v] for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy_timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--side", type=int, default=800)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    st = _lib.stream_ptr(dev)
    side, N = args.side, 128
    B = side * side
    pose = np.asarray(spherical_to_pose(4, 30, 45), dtype=np.float32)
    cam = [side, side, synthetic.focal_from_fov(side)]
    net = Nerf().to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, "structured"))
    grids = {f"ball_{r}": occupancy.OccupancyGrid.from_mask(ball_mask(r, dev), BOUNDS, outside="empty") for r in (1.0, 0.75, 0.5)}
    grids["all_live"] = occupancy.OccupancyGrid.from_mask(torch.ones((R - 1,) * 3, dtype=torch.bool, device=dev), BOUNDS)
    rays = generate_rays(pose, cam, dev)
    tb = _tbins(2, 6, N, dev)
    flags, seed = _lib.FLAG_DEVICE_RNG, 0
    res = {"device": torch.cuda.get_device_name(0), "view": {"side": side, "N": N, "rays": B, "samples": B * N},
           "grid": {"resolution": R, "bounds": BOUNDS}, "rounds": args.rounds, "precisions": {}}
    # the device-to-host read of the live count with nothing in flight: the latency floor of the sync
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    reads = []
    for _ in range(50):
        t0 = time.perf_counter()
        int(word[0])
        reads.append((time.perf_counter() - t0) * 1e3)
    res["sync_read_ms_idle_stream"] = round(statistics.median(reads), 4)

    for precision in ("fp16", "bf16"):
        code = _lib.precision_code(precision)
        packed = net.packed_weights(code)
        with torch.no_grad():
            variants = {"full": lambda: render_view(net, pose, cam, N=N, device_rng=True, seed=seed, precision=precision)}
            for name, occ in grids.items():
                variants[name] = (lambda o: lambda: render_view(net, pose, cam, N=N, device_rng=True, seed=seed,
                                                                precision=precision, occupancy=o))(occ)
            med, raw_samples = alternated(variants, args.rounds)
        out = {"T_full_ms": round(med["full"], 3), "samples_ms": raw_samples, "grids": {}}
        for name, occ in grids.items():
            m = occ.mark(rays, N, device_rng=True, seed=seed, points=True)
            P = m.live
            W = (N + 63) // 64
            ws = torch.empty(max(int(lib.nerf_amd_occupancy_workspace_bytes(B)), 256), dtype=torch.uint8, device=dev)
            mask, offsets, pts = torch.empty_like(m.mask), torch.empty_like(m.offsets), torch.empty_like(m.points)
            raw = torch.empty((max(P, 1), 4), dtype=torch.float32, device=dev)
            px = torch.empty((B, 4), dtype=torch.float32, device=dev)
            mflags = flags | (_lib.FLAG_OUTSIDE_EMPTY if occ.outside == "empty" else 0)
            lo, inv = _lib.host_f32x3(occ.lo), _lib.host_f32x3(occ.inv_step)
            stages = {
                "mark_scan": lambda: lib.nerf_amd_occupancy_mark(_lib.ptr(rays), None, _lib.ptr(tb), mflags, seed, 0, _lib.ptr(occ.words),
                                                                 *occ.resolution, lo, inv, _lib.ptr(mask), _lib.ptr(offsets), None,
                                                                 _lib.ptr(ws), B, N, st),
                "emit": lambda: lib.nerf_amd_occupancy_points(_lib.ptr(rays), None, _lib.ptr(tb), flags, seed, 0, _lib.ptr(m.mask),
                                                              _lib.ptr(m.offsets), _lib.ptr(pts), P, B, N, st),
                "network_T_pts": lambda: lib.nerf_amd_mlp_forward(_lib.ptr(m.points), _lib.ptr(packed), _lib.ptr(raw), P, code, st),
                "composite": lambda: lib.nerf_amd_volume_render_masked_pixels(_lib.ptr(raw), _lib.ptr(rays), None, _lib.ptr(tb), flags,
                                                                              seed, 0, _lib.ptr(m.mask), _lib.ptr(m.offsets),
                                                                              _lib.ptr(px), B, N, st),
            }
            smed, _ = alternated(stages, args.rounds, inner=3)
            torch.cuda.synchronize()
            assert torch.equal(mask, m.mask) and torch.equal(offsets, m.offsets) and torch.equal(pts, m.points)
            # bytes each stage moves at least (the 256 KiB of grid bits stay in L2 and are left out)
            nblk = -(-B // 2048)
            bytes_ = {"mark_scan": B * (24 + 8 * W + 4) + B * (4 + 4 + 8) + 24 * nblk,
                      "emit": B * (8 * W + 16) + (24 * B if P else 0) + 24 * P,
                      "composite": 16 * P + B * (24 + 8 * W + 16) + 16 * B}
            T_m = med[name]
            row = {"outside": occ.outside, "cell_fraction": round(occ.cell_fraction, 4), "live_samples": P,
                   "live_fraction": round(P / (B * N), 4), "T_masked_ms": round(T_m, 3),
                   "T_masked_over_T_full": round(T_m / med["full"], 4),
                   "stages_ms": {k: round(v, 4) for k, v in smed.items()},
                   "stages_sum_ms": round(sum(smed.values()), 3),
                   "T_pts_ms": round(smed["network_T_pts"], 3),
                   "overhead_T_masked_minus_T_pts_ms": round(T_m - smed["network_T_pts"], 3),
                   "stage_bytes": bytes_,
                   "stage_GBps": {k: round(bytes_[k] / (smed[k] * 1e-3) / 1e9, 1) for k in bytes_},
                   "stage_ms_at_6TBps": {k: round(bytes_[k] / 6e12 * 1e3, 4) for k in bytes_},
                   "ns_per_live_point_network": round(smed["network_T_pts"] * 1e6 / max(P, 1), 4)}
            print(json.dumps({precision: {name: row}}), flush=True)
            out["grids"][name] = row
            del ws, mask, offsets, pts, raw, px, m
            torch.cuda.empty_cache()
        # masked cost as a line in the live fraction through the radius-1 ball and the all-live grid; where it meets T_full
        a, b = out["grids"]["ball_1.0"], out["grids"]["all_live"]
        slope = (b["T_masked_ms"] - a["T_masked_ms"]) / (b["live_fraction"] - a["live_fraction"])
        fixed = a["T_masked_ms"] - slope * a["live_fraction"]
        out["masked_ms_per_unit_live_fraction"] = round(slope, 3)
        out["masked_fixed_ms"] = round(fixed, 3)
        out["break_even_live_fraction"] = round((med["full"] - fixed) / slope, 4)
        out["speedup_claim_met_T_masked_lt_half_T_full_at_ball_1.0"] = bool(a["T_masked_ms"] < 0.5 * med["full"])
        res["precisions"][precision] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
