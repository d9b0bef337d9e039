"""Time the training step through an occupancy grid against the dense eager step on one GPU
(profiles/occupancy_training_timing.json).

At 4096 rays x 64 samples, bf16, device RNG, camera spherical_to_pose(4, 30, 45) (a 64 x 64 view), t in [2, 6], structured
synthetic weights, torch.optim.SGD(lr = 0) as the optimizer so that every step does the same work on the same weights;
grids: balls of radius 1.0 / 0.75 / 0.5 in a 129^3 grid over [-1.5, 1.5]^3 with outside='empty', and the all-live grid:

  * T_dense   -- training.train_step without occupancy (the eager dense step), same process;
  * T_masked  -- training.train_step(..., occupancy=grid) end to end, its one host synchronisation included;
  * stages    -- each through the C ABI on preallocated buffers: mark + scan + the host read of the live count, emit, the
                 training forward on the P' points (with the bf16 encoder rows), the masked compositor forward and
                 backward, the dX chain, the dW products;
  * update    -- one TrainingOccupancyGrid.update() at 128^3 (density grid + decay-max + bits + the count's host read);
  * from the all-live grid and the radius-1 ball, the live fraction at which masked and dense cost the same.
The model to compare against: network stages proportional to P', plus three light passes and a host read.
HIP events around back-to-back calls after a warm-up; the variants are ALTERNATED round by round and the median over the
rounds is reported (the eager steps are host-bound at this size: wall clock between synchronisations is reported too).

usage: python tools/time_occupancy_training.py [--out profiles/occupancy_training_timing.json] [--rounds 7]     (GPU box)
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
from nerf_simple_amd.training import train_step  # noqa: E402
from nerf_simple_amd.utils import occupancy, synthetic  # noqa: E402
from nerf_simple_amd.utils.nets import Nerf  # noqa: E402
from nerf_simple_amd.utils.rendering import _tbins, generate_rays  # noqa: E402
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


def wall_ms(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def alternated(variants, rounds, inner, timer=event_ms):
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            samples[k].append(timer(fn, inner))
    return {k: statistics.median(v) for k, v in samples.items()}, {k: [round(x, 3) for x in v] for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy_training_timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--end-to-end", default=None, help="JSON report of the end-to-end test to fold in (per-seed PSNRs etc.)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    st = _lib.stream_ptr(dev)
    side, N = 64, 64
    B = side * side
    pose = np.asarray(spherical_to_pose(4, 30, 45), dtype=np.float32)
    rays = generate_rays(pose, [side, side, synthetic.focal_from_fov(side)], dev)
    gt = torch.rand(B, 3, device=dev)
    net = Nerf(precision="bf16").to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, "structured"))
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    grids = {f"ball_{r}": occupancy.OccupancyGrid.from_mask(ball_mask(r, dev), BOUNDS, outside="empty") for r in (1.0, 0.75, 0.5)}
    grids["all_live"] = occupancy.OccupancyGrid.from_mask(torch.ones((R - 1,) * 3, dtype=torch.bool, device=dev), BOUNDS)
    tb = _tbins(2, 6, N, dev)
    flags, seed = _lib.FLAG_DEVICE_RNG, 0
    res = {"device": torch.cuda.get_device_name(0), "step": {"rays": B, "N": N, "samples": B * N, "precision": "bf16"},
           "grid": {"resolution": R, "bounds": BOUNDS}, "rounds": args.rounds}

    # ---- whole steps, alternated ----
    steps = {"dense": lambda: train_step(net, opt, rays, gt, N, device_rng=True, seed=seed)}
    for name, occ in grids.items():
        steps[name] = (lambda o: lambda: train_step(net, opt, rays, gt, N, device_rng=True, seed=seed, occupancy=o))(occ)
    med, samples = alternated(steps, args.rounds, inner=5)
    wall, _ = alternated(steps, args.rounds, inner=5, timer=wall_ms)
    res["T_dense_ms"] = round(med["dense"], 3)
    res["T_dense_wall_ms"] = round(wall["dense"], 3)
    res["step_samples_ms"] = samples
    res["grids"] = {}

    # ---- stages through the C ABI ----
    packed, image = net.packed_weights(_lib.BF16), net.packed_weights(_lib.BF16_BWD)
    for name, occ in grids.items():
        m = occ.mark(rays, N, device_rng=True, seed=seed, points=True)
        P = m.live
        ws = torch.empty(max(int(lib.nerf_amd_occupancy_workspace_bytes(B)), 256), dtype=torch.uint8, device=dev)
        mask, offsets, pts = torch.empty_like(m.mask), torch.empty_like(m.offsets), torch.empty_like(m.points)
        raw = torch.empty((P, 4), dtype=torch.float32, device=dev)
        d_raw = torch.empty_like(raw)
        acts = torch.empty(int(lib.nerf_amd_train_activation_bytes(P)), dtype=torch.uint8, device=dev)
        dys = torch.empty_like(acts)
        posx = torch.empty((P, 64), dtype=torch.bfloat16, device=dev)
        posd = torch.empty((P, 32), dtype=torch.bfloat16, device=dev)
        flat = torch.empty(int(lib.nerf_amd_param_count()), dtype=torch.float32, device=dev)
        scratch = torch.empty(max(int(lib.nerf_amd_param_gradients_scratch_bytes(P)), 16), dtype=torch.uint8, device=dev)
        rgb, disp, acc = (torch.empty(s, dtype=torch.float32, device=dev) for s in ((B, 3), (B,), (B,)))
        g_rgb = torch.randn(B, 3, device=dev) / B
        mflags = flags | (_lib.FLAG_OUTSIDE_EMPTY if occ.outside == "empty" else 0)
        lo, inv = _lib.host_f32x3(occ.lo), _lib.host_f32x3(occ.inv_step)
        head = (_lib.ptr(rays), None, _lib.ptr(tb), flags, seed, 0, _lib.ptr(m.mask), _lib.ptr(m.offsets))

        def mark_scan_read():
            lib.nerf_amd_occupancy_mark(_lib.ptr(rays), None, _lib.ptr(tb), mflags, seed, 0, _lib.ptr(occ.words), *occ.resolution, lo,
                                        inv, _lib.ptr(mask), _lib.ptr(offsets), None, _lib.ptr(ws), B, N, st)
            return int(offsets[B])

        def forward():
            lib.nerf_amd_mlp_forward_train_points(_lib.ptr(pts), _lib.ptr(packed), _lib.ptr(raw), _lib.ptr(acts), P, st)
            lib.nerf_amd_encode_points_bf16(_lib.ptr(pts), _lib.ptr(posx), _lib.ptr(posd), P, st)

        stages = {
            "mark_scan_read": mark_scan_read,
            "emit": lambda: lib.nerf_amd_occupancy_points(_lib.ptr(rays), None, _lib.ptr(tb), flags, seed, 0, _lib.ptr(m.mask),
                                                          _lib.ptr(m.offsets), _lib.ptr(pts), P, B, N, st),
            "forward": forward,
            "composite_forward": lambda: lib.nerf_amd_volume_render_masked(_lib.ptr(raw), *head, _lib.ptr(rgb), _lib.ptr(disp), None,
                                                                          _lib.ptr(acc), None, B, N, st),
            "composite_backward": lambda: lib.nerf_amd_volume_render_masked_backward(_lib.ptr(raw), *head, _lib.ptr(g_rgb), None, None,
                                                                                    None, None, _lib.ptr(d_raw), B, N, st),
            "dX": lambda: lib.nerf_amd_mlp_backward(_lib.ptr(d_raw), _lib.ptr(image), _lib.ptr(acts), _lib.ptr(dys), P, st),
            "dW": lambda: lib.nerf_amd_param_gradients(_lib.ptr(d_raw), _lib.ptr(acts), _lib.ptr(dys), _lib.ptr(posx), _lib.ptr(posd),
                                                       _lib.ptr(scratch), _lib.ptr(flat), P, st),
        }
        smed, _ = alternated(stages, args.rounds, inner=3)
        torch.cuda.synchronize()
        assert torch.equal(mask, m.mask) and torch.equal(offsets, m.offsets) and torch.equal(pts, m.points)
        network = smed["forward"] + smed["dX"] + smed["dW"]
        light = smed["mark_scan_read"] + smed["emit"] + smed["composite_forward"] + smed["composite_backward"]
        row = {"outside": occ.outside, "cell_fraction": round(occ.cell_fraction, 4), "live_samples": P,
               "live_fraction": round(P / (B * N), 4), "T_masked_ms": round(med[name], 3),
               "T_masked_wall_ms": round(wall[name], 3), "T_masked_over_T_dense": round(med[name] / med["dense"], 4),
               "stages_ms": {k: round(v, 4) for k, v in smed.items()}, "network_stages_ms": round(network, 4),
               "light_stages_ms": round(light, 4), "stages_sum_ms": round(network + light, 4),
               "ns_per_live_point_network": round(network * 1e6 / max(P, 1), 3)}
        print(json.dumps({name: row}), flush=True)
        res["grids"][name] = row
    a, b = res["grids"]["ball_1.0"], res["grids"]["all_live"]
    for key, tag in (("T_masked_ms", ""), ("stages_sum_ms", "_device_stages")):
        slope = (b[key] - a[key]) / (b["live_fraction"] - a["live_fraction"])
        fixed = a[key] - slope * a["live_fraction"]
        res["masked_ms_per_unit_live_fraction" + tag] = round(slope, 3)
        res["masked_fixed_ms" + tag] = round(fixed, 3)
    slope, fixed = res["masked_ms_per_unit_live_fraction"], res["masked_fixed_ms"]
    res["break_even_live_fraction"] = round((med["dense"] - fixed) / slope, 4) if slope > 0 else None

    # ---- one update at 128^3 ----
    tog = occupancy.TrainingOccupancyGrid(128, BOUNDS, outside="empty", device=dev)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        umed, _ = alternated({"update_128": lambda: tog.update(net, level=-1.75)}, args.rounds, inner=1, timer=wall_ms)
    res["update_128_ms"] = round(umed["update_128"], 3)
    res["update_128_cell_fraction"] = round(tog.cell_fraction, 4)
    if args.end_to_end and os.path.exists(args.end_to_end):
        with open(args.end_to_end) as fh:
            res["end_to_end"] = json.load(fh)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
