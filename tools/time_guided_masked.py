"""Timing of guided sampling through an occupancy grid next to what it replaces or competes with.  All
variants of a group run in ONE process, alternating, and the median of 5 timed rounds (HIP events, after warm-up) is reported
with min ... max, as tools/time_guided.py does:

  * placement: nerf_amd_sample_pdf_volume_masked at 640,000 rays x (64 + 128), 128^3 volume, 128^3 ball grid, next to the three
               launches it replaces (nerf_amd_sample_pdf_volume + nerf_amd_occupancy_mark on the coarse jitter and on ts).  The
               chain does not mask the coarse samples, so its positions differ: the live fraction of both is recorded;
  * render:    one 800 x 800 view at 64 + 128, fp16, counter RNG, radius-1 ball: render_guided_view dense and with the grid,
               and render_hierarchical_view(occupancy=);
  * step:      at 4096 rays x (64 + 128) on the radius-1 ball with a tight capacity (largest live count of 8 eager steps plus
               a 256-row margin): GraphedGuidedTrainStep, GraphedMaskedGuidedTrainStep, GraphedMaskedHierarchicalTrainStep;
               and the live fraction of the merged samples with and without the coarse masking.

Writes profiles/guided_masked_timing.json.  The baselines are entry points this feature does not touch."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_simple_amd import _lib                                                                     # noqa: E402
from nerf_simple_amd.optim import FusedAdam                                                          # noqa: E402
from nerf_simple_amd.training import (GraphedGuidedTrainStep, GraphedMaskedGuidedTrainStep,          # noqa: E402
                                      GraphedMaskedHierarchicalTrainStep, train_step_guided, train_step_hierarchical)
from nerf_simple_amd.utils import synthetic                                                          # noqa: E402
from nerf_simple_amd.utils.nets import Nerf                                                          # noqa: E402
from nerf_simple_amd.utils.occupancy import OccupancyGrid                                            # noqa: E402
from nerf_simple_amd.utils.proposal import ProposalVolume                                            # noqa: E402
from nerf_simple_amd.utils.rendering import generate_rays, render_guided_view, render_hierarchical_view      # noqa: E402
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


def net_on(dev, seed, kind="structured"):
    n = Nerf(precision="bf16").to(dev)
    n.load_state_dict(synthetic.synthetic_state_dict(seed, kind))
    return n


def ball_grid(R, radius, dev):
    c = (torch.arange(R - 1, dtype=torch.float64, device=dev) + 0.5) * (3.0 / (R - 1)) - 1.5
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    return OccupancyGrid.from_mask(X * X + Y * Y + Z * Z <= radius * radius, BOUNDS, outside="empty")


def up256(n, total):
    return min(-(-(n + 256) // 256) * 256, total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--Nc", type=int, default=64)
    ap.add_argument("--Nf", type=int, default=128)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_masked_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    Nc, Nf, N, runs = args.Nc, args.Nf, args.Nc + args.Nf, args.runs
    lib, ptr = _lib.lib(), _lib.ptr
    net_c, net_f = net_on(dev, 0), net_on(dev, 1)
    prop = ProposalVolume(args.resolution, BOUNDS, device=dev).update(net_f)
    occ = ball_grid(args.resolution, args.radius, dev)
    out = {"config": {"view": [args.side, args.side], "train_rays": args.rays, "Nc": Nc, "Nf": Nf, "resolution": args.resolution,
                      "grid": {"resolution": args.resolution, "ball_radius": args.radius, "outside": occ.outside,
                               "cell_fraction": round(occ.cell_fraction, 4)},
                      "runs": runs, "device": torch.cuda.get_device_name(dev)}}

    # ---- the placement alone: one entry point against the three launches it replaces ----
    pose = spherical_to_pose(4, -30, 0)
    cam = (args.side, args.side, synthetic.focal_from_fov(args.side))
    rays = generate_rays(pose, cam, dev)
    B = rays.shape[0]
    tbins = torch.linspace(2, 6, Nc + 1).to(dev)
    i64 = dict(dtype=torch.int64, device=dev)
    ts_a, ts_b = (torch.empty((B, N), dtype=torch.float32, device=dev) for _ in range(2))
    mask_a, mask_b = (torch.empty((B, (N + 63) // 64), **i64) for _ in range(2))
    mask_c = torch.empty((B, (Nc + 63) // 64), **i64)
    off_a, off_b, off_c = (torch.empty(B + 1, **i64) for _ in range(3))
    ws = torch.empty(max(int(lib.nerf_amd_occupancy_workspace_bytes(B)), 256), dtype=torch.uint8, device=dev)
    RNG, GIVEN, EMPTY = _lib.FLAG_DEVICE_RNG, _lib.FLAG_TS_GIVEN, _lib.FLAG_OUTSIDE_EMPTY
    g_lo, g_inv, st = _lib.host_f32x3(occ.lo), _lib.host_f32x3(occ.inv_step), _lib.stream_ptr(dev)

    def masked():
        prop._launch_masked(occ, rays, None, tbins, RNG, 1, 0, None, ts_a, None, None, mask_a, off_a, None, ws, B, Nc, Nf)

    def mark(jit, tb, flags, mask, offsets, n):
        _lib.check(lib.nerf_amd_occupancy_mark(ptr(rays), ptr(jit), ptr(tb), flags | EMPTY, 1, 0, ptr(occ.words), *occ.resolution,
                                               g_lo, g_inv, ptr(mask), ptr(offsets), None, ptr(ws), B, n, st), "mark")

    def chain():
        prop._launch(rays, None, tbins, RNG, 1, 0, None, ts_b, None, None, B, Nc, Nf)
        mark(None, tbins, RNG, mask_c, off_c, Nc)
        mark(ts_b, None, GIVEN, mask_b, off_b, N)

    def unmasked_placement():
        prop._launch(rays, None, tbins, RNG, 1, 0, None, ts_b, None, None, B, Nc, Nf)

    with torch.cuda.device(dev):
        out["placement"] = alternate({"nerf_amd_sample_pdf_volume_masked": masked,
                                      "nerf_amd_sample_pdf_volume + nerf_amd_occupancy_mark x2": chain,
                                      "nerf_amd_sample_pdf_volume": unmasked_placement}, runs, 10, 3)
    torch.cuda.synchronize()
    out["placement"]["rays"] = B
    out["placement"]["live_fraction"] = {"coarse": round(int(off_c[B]) / (B * Nc), 4),
                                         "merged, coarse samples masked (the entry point)": round(int(off_a[B]) / (B * N), 4),
                                         "merged, not masked (the chain)": round(int(off_b[B]) / (B * N), 4)}

    # ---- one view ----
    kw = dict(device_rng=True, precision="fp16")
    with torch.no_grad():
        out["render"] = alternate({
            "render_guided_view": lambda: render_guided_view(net_f, pose, cam, Nc, Nf, prop, **kw),
            "render_guided_view(occupancy=)": lambda: render_guided_view(net_f, pose, cam, Nc, Nf, prop, occupancy=occ, **kw),
            "render_hierarchical_view(occupancy=)": lambda: render_hierarchical_view(net_c, net_f, pose, cam, Nc, Nf,
                                                                                     occupancy=occ, **kw)}, runs, 3, 2)
        render_guided_view(net_f, pose, cam, Nc, Nf, prop, occupancy=occ, **kw)
        out["render"]["render_guided_view(occupancy=)"]["live_fraction"] = round(occ.last_stats["live"] / (B * N), 4)
        render_hierarchical_view(net_c, net_f, pose, cam, Nc, Nf, occupancy=occ, **kw)
        s_ = occ.last_stats
        out["render"]["render_hierarchical_view(occupancy=)"]["live_fraction"] = {
            "coarse": round(s_["coarse"]["live"] / (B * Nc), 4), "fine": round(s_["fine"]["live"] / (B * N), 4)}

    # ---- the graphed training step (lr = 0: the live counts of the timed steps are those measured below) ----
    Bt = args.rays
    g = torch.Generator().manual_seed(0)
    sel = torch.randperm(B, generator=g)[:Bt].to(dev)
    trays, gt = rays[sel].contiguous(), torch.rand(Bt, 3, generator=g).to(dev)
    a, b, c, d, e = (net_on(dev, s) for s in (1, 1, 0, 1, 1))
    seed, steps = 7, 8
    opt_e = FusedAdam(e, lr=0.0)
    live_g = live_plain = 0
    for k in range(1, steps + 1):
        train_step_guided(e, opt_e, trays, gt, Nc, Nf, prop, device_rng=True, seed=seed + k, occupancy=occ)
        live_g = max(live_g, occ.last_stats["live"])
        ts = prop.sample(trays, Nc, Nf, device_rng=True, seed=seed + k)
        live_plain = max(live_plain, occ.mark(trays, N, ts=ts).live)
    pair_opt = torch.optim.SGD(list(c.parameters()) + list(d.parameters()), lr=0.0)
    live_hc = live_hf = 0
    for k in range(1, steps + 1):
        train_step_hierarchical(c, d, pair_opt, trays, gt, Nc, Nf, device_rng=True, seed=seed + k, occupancy=occ)
        live_hc, live_hf = max(live_hc, occ.last_stats["coarse"]["live"]), max(live_hf, occ.last_stats["fine"]["live"])
    C_g, C_h = up256(live_g, Bt * N), (up256(live_hc, Bt * Nc), up256(live_hf, Bt * N))
    steppers = {
        "GraphedGuidedTrainStep": GraphedGuidedTrainStep(a, FusedAdam(a, lr=0.0), Bt, Nc, Nf, prop, device_rng=True, seed=seed,
                                                         check_every=0),
        "GraphedMaskedGuidedTrainStep": GraphedMaskedGuidedTrainStep(b, FusedAdam(b, lr=0.0), Bt, Nc, Nf, prop, occ, C_g,
                                                                     device_rng=True, seed=seed, check_every=0),
        "GraphedMaskedHierarchicalTrainStep": GraphedMaskedHierarchicalTrainStep(c, d, FusedAdam([c, d], lr=0.0), Bt, Nc, Nf, occ,
                                                                                 C_h, device_rng=True, seed=seed, check_every=0)}
    out["step"] = alternate({k: (lambda s=s: s.step(trays, gt)) for k, s in steppers.items()}, runs, 50, 10)
    cg, ch = steppers["GraphedMaskedGuidedTrainStep"].counts(), steppers["GraphedMaskedHierarchicalTrainStep"].counts()
    out["step"]["GraphedMaskedGuidedTrainStep"].update(
        capacity=C_g, capacity_fraction=round(C_g / (Bt * N), 4), live_last_step=cg["live"], overflowed=cg["live"] > cg["capacity"])
    out["step"]["GraphedMaskedHierarchicalTrainStep"].update(
        capacity=list(C_h), capacity_fraction=[round(C_h[0] / (Bt * Nc), 4), round(C_h[1] / (Bt * N), 4)],
        live_last_step=[ch["coarse"]["live"], ch["fine"]["live"]],
        overflowed=ch["coarse"]["live"] > ch["coarse"]["capacity"] or ch["fine"]["live"] > ch["fine"]["capacity"])
    out["step"]["merged_live_fraction_max_of_8_steps"] = {"coarse samples masked": round(live_g / (Bt * N), 4),
                                                          "not masked": round(live_plain / (Bt * N), 4)}

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
