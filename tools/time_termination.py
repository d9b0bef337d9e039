"""Time early ray termination against the dense and the masked render on one GPU (profiles/termination_timing.json).

At 800 x 800 x 128, camera spherical_to_pose(4, -30, 40), t in [2, 6], device RNG, fp16, one process:

  * variants  -- the dense render_view; the masked render_view(..., occupancy=grid); the terminated
                 render_view(..., occupancy=grid, terminate=EarlyTermination(eps, S)) for S in {16, 32, 64} x
                 eps in {1e-4, 1e-3, 1e-2}; ALTERNATED round by round (as tools/time_occupancy.py does), median reported;
  * grids     -- the all-live grid, and the radius-1 ball in a 129^3 grid over [-1.5, 1.5]^3 with outside='empty';
  * weights   -- the `structured` synthetic set, and the same set with sigma_fc.0.bias raised by SIGMA_SHIFT = 8.0: on the CPU
                 oracle (20 x 20 rays of this view, N = 128, S = 16) 87 / 75 / 65 % of the rays through the ball then terminate
                 inside it at eps = 1e-2 / 1e-3 / 1e-4, against 2 / 0 / 0 % without the shift;
  * per terminated variant -- the evaluated-sample fraction, the host reads, the slabs run and the network launches
                 (EarlyTermination.last_stats), the time of the whole call, and the time per stage: the loop of
                 utils/occupancy.render_terminated replayed through the C ABI with HIP events around every stage (mark + scan,
                 advance, emit, network, composite; what is left of the wall clock is the host: reads, allocation, launches).
                 The stage times therefore come from a pass of their own (`staged_pass_wall_ms`), not from the alternated calls
                 behind `T_ms`, and exist for the terminated variants only: the dense render is one kernel, and the masked
                 render's stage split is what tools/time_occupancy.py records (profiles/occupancy_timing.json).

A record, not a criterion: no test asserts a time.

usage: python tools/time_termination.py [--out profiles/termination_timing.json] [--rounds 5] [--side 800]     (GPU box)
"""
import argparse
import ctypes
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
SIGMA_SHIFT = 8.0
SLABS = (16, 32, 64)
EPS = (1e-4, 1e-3, 1e-2)


def ball_mask(radius, dev):
    c = (torch.arange(R - 1, dtype=torch.float64, device=dev) + 0.5) * (3.0 / (R - 1)) - 1.5
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    return X * X + Y * Y + Z * Z <= radius * radius


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternated(variants, rounds):
    """{name: median ms per call, host wall clock with a device synchronisation at both ends}: one warm-up pass, then
    `rounds` passes over all variants in turn (the terminated render waits for the device inside the call, so the wall
    clock is the honest measure for all of them)"""
    for fn in variants.values():
        fn()
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            samples[k].append(wall_ms(fn))
    return {k: statistics.median(v) for k, v in samples.items()}, {k: [round(x, 3) for x in v] for k, v in samples.items()}


class Stages:
    """HIP events around the stages of one pass; ms per stage after a synchronisation"""

    def __init__(self):
        self.spans = []

    def run(self, name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self.spans.append((name, a, b))
        return out

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.spans:
            out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        return out


def staged_pass(lib, dev, occ, rays, tb, seed, packed, code, eps, S, N):
    """the loop of utils/occupancy.render_terminated through the C ABI, every stage between two events"""
    B = rays.shape[0]
    st = _lib.stream_ptr(dev)
    K, W = -(-N // S), (N + 63) // 64
    flags = _lib.FLAG_DEVICE_RNG
    head = (_lib.ptr(rays), None, _lib.ptr(tb), flags, seed, 0)
    sg = Stages()
    t0 = time.perf_counter()
    m = sg.run("mark_scan", lambda: occupancy._mark(occ, rays, None, tb, flags, seed, 0, N))
    raw0 = torch.tensor([0.0, 0.0, 0.0, -np.inf], device=dev).repeat(max(m.live, 1), 1)
    trans = torch.ones((B, K), dtype=torch.float32, device=dev)
    masks = [torch.empty((B, W), dtype=torch.int64, device=dev) for _ in range(2)]
    offs = [torch.empty(B + 1, dtype=torch.int64, device=dev) for _ in range(2)]
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(lib.nerf_amd_termination_workspace_bytes(B)), 256), dtype=torch.uint8, device=dev)

    def advance(raw, cur, rows, s0, s1, s2):
        _lib.check(lib.nerf_amd_termination_advance(
            _lib.ptr(raw), _lib.ptr(masks[cur]) if raw is not None else None, _lib.ptr(offs[cur]) if raw is not None else None, rows,
            *head, _lib.ptr(m.mask), _lib.ptr(m.offsets), _lib.ptr(raw0), m.live, ctypes.c_float(eps), S, s0, s1, s2, _lib.ptr(trans),
            _lib.ptr(masks[1 - cur]), _lib.ptr(offs[1 - cur]), _lib.ptr(totals), _lib.ptr(ws), B, N, st), "advance")

    sg.run("advance", lambda: advance(None, 1, 0, 0, 0, min(S, N)))
    cur, evaluated, reads = 0, 0, 1
    for k in range(K):
        count, remaining = totals.tolist()
        reads += 1
        if remaining == 0:
            break
        raw = None
        if count:
            pts = torch.empty((count, 6), dtype=torch.float32, device=dev)
            raw = torch.empty((count, 4), dtype=torch.float32, device=dev)
            sg.run("emit", lambda: _lib.check(lib.nerf_amd_occupancy_points(*head, _lib.ptr(masks[cur]), _lib.ptr(offs[cur]),
                                                                            _lib.ptr(pts), count, B, N, st), "emit"))
            sg.run("network", lambda: _lib.check(lib.nerf_amd_mlp_forward(_lib.ptr(pts), _lib.ptr(packed), _lib.ptr(raw), count, code,
                                                                          st), "forward"))
            evaluated += count
        s1 = min(k * S + S, N)
        sg.run("advance", lambda: advance(raw, cur, count, k * S, s1, min(s1 + S, N)))
        cur = 1 - cur
    px = torch.empty((B, 4), dtype=torch.float32, device=dev)
    sg.run("composite", lambda: _lib.check(lib.nerf_amd_volume_render_masked_pixels(
        _lib.ptr(raw0), *head, _lib.ptr(m.mask), _lib.ptr(m.offsets), _lib.ptr(px), B, N, st), "composite"))
    stages = sg.totals()
    wall = (time.perf_counter() - t0) * 1e3
    stages = {k: round(v, 3) for k, v in stages.items()}
    stages["host_and_idle"] = round(wall - sum(stages.values()), 3)
    return stages, round(wall, 3), evaluated, reads, px


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "termination_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--side", type=int, default=800)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    side, N, precision, seed = args.side, 128, "fp16", 0
    B = side * side
    code = _lib.precision_code(precision)
    pose = np.asarray(spherical_to_pose(4, -30, 40), dtype=np.float32)
    cam = [side, side, synthetic.focal_from_fov(side)]
    rays = generate_rays(pose, cam, dev)
    tb = _tbins(2, 6, N, dev)
    grids = {"all_live": occupancy.OccupancyGrid.from_mask(torch.ones((R - 1,) * 3, dtype=torch.bool, device=dev), BOUNDS),
             "ball_1.0": occupancy.OccupancyGrid.from_mask(ball_mask(1.0, dev), BOUNDS, outside="empty")}
    res = {"device": torch.cuda.get_device_name(0), "precision": precision,
           "view": {"side": side, "N": N, "rays": B, "samples": B * N, "pose": "spherical_to_pose(4, -30, 40)"},
           "grid": {"resolution": R, "bounds": BOUNDS}, "rounds": args.rounds, "sigma_shift": SIGMA_SHIFT,
           "timing": "host wall clock, device synchronised at both ends, median over alternated rounds",
           "stages_note": "stages_ms / host_and_idle come from ONE separate replay of the loop through the C ABI with HIP events "
                          "around every stage (staged_pass_wall_ms is that pass's wall clock), not from the calls behind T_ms; "
                          "recorded for the terminated variants only (dense: one kernel; masked: tools/time_occupancy.py)",
           "weights": {}}
    for wname, shift in (("structured", 0.0), (f"structured_sigma_bias_plus_{SIGMA_SHIFT:g}", SIGMA_SHIFT)):
        sd = {k: v.clone() for k, v in synthetic.synthetic_state_dict(0, "structured").items()}
        sd["sigma_fc.0.bias"] += shift
        net = Nerf(precision=precision).to(dev)
        net.load_state_dict(sd)
        packed = net.packed_weights(code)
        out = {}
        with torch.no_grad():
            for gname, occ in grids.items():
                terms = {(S, eps): occupancy.EarlyTermination(eps, S) for S in SLABS for eps in EPS}
                variants = {"dense": lambda: render_view(net, pose, cam, N=N, device_rng=True, seed=seed, precision=precision),
                            "masked": lambda: render_view(net, pose, cam, N=N, device_rng=True, seed=seed, precision=precision,
                                                          occupancy=occ)}
                for key, term in terms.items():
                    variants[f"S{key[0]}_eps{key[1]:g}"] = (lambda t: lambda: render_view(
                        net, pose, cam, N=N, device_rng=True, seed=seed, precision=precision, occupancy=occ, terminate=t))(term)
                med, samples = alternated(variants, args.rounds)
                live = occ.last_stats["live"] if "live" in occ.last_stats else None
                row = {"T_dense_ms": round(med["dense"], 3), "T_masked_ms": round(med["masked"], 3), "terminated": {}, "samples_ms": samples}
                for key, term in terms.items():
                    name = f"S{key[0]}_eps{key[1]:g}"
                    stt = term.last_stats
                    stages, wall, evaluated, reads, px = staged_pass(lib, dev, occ, rays, tb, seed, packed, code, term.eps, term.slab, N)
                    assert evaluated == stt["evaluated"] and reads == stt["host_reads"], (name, evaluated, stt)
                    row["terminated"][name] = {
                        "slab": key[0], "eps": key[1], "T_ms": round(med[name], 3),
                        "over_dense": round(med[name] / med["dense"], 4), "over_masked": round(med[name] / med["masked"], 4),
                        "live": stt["live"], "evaluated": stt["evaluated"],
                        "evaluated_fraction_of_live": round(stt["evaluated"] / max(stt["live"], 1), 4),
                        "evaluated_fraction_of_samples": round(stt["evaluated"] / (B * N), 4),
                        "terminated_rays_fraction": round(stt["terminated_rays"] / B, 4),
                        "host_reads": stt["host_reads"], "slabs_run": stt["slabs_run"], "network_launches": stt["network_launches"],
                        "stages_ms": stages, "staged_pass_wall_ms": wall}
                    print(json.dumps({wname: {gname: {name: row["terminated"][name]}}}), flush=True)
                best = min(row["terminated"], key=lambda k: row["terminated"][k]["T_ms"])
                row["fastest_terminated"] = best
                row["fastest_terminated_beats_masked"] = bool(row["terminated"][best]["T_ms"] < med["masked"])
                row["fastest_terminated_beats_dense"] = bool(row["terminated"][best]["T_ms"] < med["dense"])
                print(json.dumps({wname: {gname: {k: row[k] for k in ("T_dense_ms", "T_masked_ms", "fastest_terminated")}}}), flush=True)
                out[gname] = row
                torch.cuda.empty_cache()
        res["weights"][wname] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
