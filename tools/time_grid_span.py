"""Timing of the grid span on the radius-1 ball in a 129^3 grid and the lego camera (distance 4, tn = 2,
tf = 6), beside no placement and the live cells' box (``SceneBox.from_occupancy``).  All variants of a group run in ONE
process, alternating, and the median of 5 timed rounds (HIP events, after warm-up) is reported with min ... max, as
tools/time_box.py does:

  * placement:  nerf_amd_span_positions alone at 640,000 x 128 and 4096 x 64, next to nerf_amd_box_positions on the same rays;
  * masked:     GraphedMaskedTrainStep at N = 64, GraphedMaskedBoxTrainStep with the live cells' box and the same stepper with
                the span, each placement at the N that gives (about) the plain step's live samples per ray that meets a live
                cell, capacities 1.1 x the batch's live count; ``counts()`` of the last step is recorded beside each;
  * view:       render_view at 800 x 800 through the grid, fp16: N = 128 plain, and the box and the span at matching density.

Nothing here fixes a threshold: a row where the span does not pay says so (``vs_plain_ms`` > 0).  lr = 0.  The live counts are
counts, not quality: no trained scene is involved.  Writes profiles/grid_span_timing.json."""
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
from nerf_simple_amd.training import GraphedMaskedBoxTrainStep, GraphedMaskedTrainStep               # noqa: E402
from nerf_simple_amd.utils import synthetic                                                          # noqa: E402
from nerf_simple_amd.utils.box import GridSpan, SceneBox                                             # noqa: E402
from nerf_simple_amd.utils.rendering import generate_rays, render_view                               # noqa: E402
from nerf_simple_amd.utils.xyz import spherical_to_pose                                              # noqa: E402
from time_masked_controls import against, alternate, ball_grid, net_on                               # noqa: E402


def batch_stats(box, occ, rays, N, seed, hit):
    """live samples of one batch under a placement, and per ray of ``hit`` (the rays that meet a live cell)"""
    ts = None if box is None else box.positions(rays, N, device_rng=True, seed=seed)
    m = occ.mark(rays, N, device_rng=True, seed=seed) if ts is None else occ.mark(rays, N, ts=ts)
    return {"N": N, "live": m.live, "live_share": round(m.live / (rays.shape[0] * N), 4), "live_per_hit_ray": round(m.live / hit, 2)}


def matching_n(box, occ, rays, seed, hit, target, n_max):
    """the smallest multiple of 2 at which the placement's live samples per hit ray reach ``target``"""
    for n in range(2, n_max + 1, 2):
        if batch_stats(box, occ, rays, n, seed, hit)["live_per_hit_ray"] >= target:
            return n
    return n_max


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--view-N", type=int, default=128)
    ap.add_argument("--resolution", type=int, default=129)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_span_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    B, N, runs = args.rays, args.N, args.runs
    occ = ball_grid(args.resolution, args.radius, dev)
    span, tight = GridSpan(occ), SceneBox.from_occupancy(occ)
    placements = {"plain": None, "live cells' box": tight, "grid span": span}
    pose, cam = spherical_to_pose(4, -30, 0), (args.side, args.side, synthetic.focal_from_fov(args.side))
    g = torch.Generator().manual_seed(0)
    view = generate_rays(pose, cam, dev)
    rays = view[torch.randperm(view.shape[0], generator=g)[:B].to(dev)].contiguous()
    gt = torch.rand(B, 3, generator=g).to(dev)
    out = {"config": {"rays": B, "N": N, "view": [args.side, args.side, args.view_N], "tn": 2, "tf": 6, "probes": span.probes,
                      "grid": {"resolution": args.resolution, "ball_radius": args.radius, "outside": occ.outside,
                               "cell_fraction": round(occ.cell_fraction, 4)},
                      "box": {"lo": tight.lo, "hi": tight.hi}, "runs": runs, "device": torch.cuda.get_device_name(dev)}}

    # ---- (a) the placement kernels alone, counter RNG ----
    out["placement"] = {}
    for r, n, reps in ((view, args.view_N, 20), (rays, N, 200)):
        rows = r.shape[0]
        ts = torch.empty((rows, n), dtype=torch.float32, device=dev)
        tb01 = torch.linspace(0, 1, n + 1).to(dev)
        head = (_lib.ptr(r), None, _lib.ptr(tb01), _lib.FLAG_DEVICE_RNG, 3, 0)
        tail = (2.0, 6.0, _lib.ptr(ts), None, None, rows, n, _lib.stream_ptr(dev))
        calls = {"nerf_amd_box_positions": (*head, _lib.host_f32x3(tight.lo), _lib.host_f32x3(tight.hi), *tail),
                 "nerf_amd_span_positions": (*head, _lib.ptr(occ.words), *occ.resolution, _lib.host_f32x3(occ.lo),
                                             _lib.host_f32x3(occ.bounds[1]), _lib.host_f32x3(occ.inv_step), span.probes, *tail)}
        table = alternate({k: (lambda k=k, c=c: _lib.check(getattr(_lib.lib(), k)(*c), k)) for k, c in calls.items()}, runs, reps, 5)
        hit = int(span.positions(r, n, device_rng=True, seed=3, return_span=True)[2].sum())
        table["rays_with_a_live_cell"] = hit
        table["note"] = "back-to-back eager launches into one preallocated buffer: at the small size this is the launch rate"
        out["placement"][f"{rows} x {n}"] = table

    # ---- (b) the masked step at matching density ----
    hit = int(span.positions(rays, N, device_rng=True, seed=8, return_span=True)[2].sum())
    target = batch_stats(None, occ, rays, N, 8, hit)["live_per_hit_ray"]
    ns = {"plain": N, "live cells' box": matching_n(tight, occ, rays, 8, hit, target, N), "grid span": matching_n(span, occ, rays, 8, hit, target, N)}
    steppers, batches = {}, {}
    for k, b in placements.items():
        batches[k] = batch_stats(b, occ, rays, ns[k], 8, hit)
        cap = min(-(-int(1.1 * batches[k]["live"]) // 256) * 256, B * ns[k])
        net = net_on(dev)
        opt = FusedAdam(net, lr=0.0)
        kw = dict(device_rng=True, seed=7, check_every=0)
        steppers[k] = (GraphedMaskedTrainStep(net, opt, B, ns[k], occ, cap, **kw) if b is None else
                       GraphedMaskedBoxTrainStep(net, opt, B, ns[k], b, occ, cap, **kw))
    out["masked"] = against(alternate({k: (lambda s=s: s.step(rays, gt)) for k, s in steppers.items()}, runs, 50, 10), "plain")
    out["masked"]["rays_with_a_live_cell"] = hit
    for k, s in steppers.items():
        cnt = s.counts()
        out["masked"][k].update(batch=batches[k], counts_last_step=cnt, overflowed=cnt["live"] > cnt["capacity"],
                                live_per_hit_ray_last_step=round(cnt["live"] / hit, 2))
    del steppers

    # ---- (c) render_view through the grid at matching density ----
    vnet = net_on(dev)
    vhit = int(span.positions(view, args.view_N, device_rng=True, seed=5, return_span=True)[2].sum())
    vtarget = batch_stats(None, occ, view, args.view_N, 5, vhit)["live_per_hit_ray"]
    vns = {"plain": args.view_N, "live cells' box": matching_n(tight, occ, view, 5, vhit, vtarget, args.view_N),
           "grid span": matching_n(span, occ, view, 5, vhit, vtarget, args.view_N)}
    with torch.no_grad():
        variants = {k: (lambda k=k, b=b: render_view(vnet, pose, cam, N=vns[k], device_rng=True, seed=5, occupancy=occ, precision="fp16",
                                                     **({} if b is None else {"box": b}))) for k, b in placements.items()}
        out["view"] = against(alternate(variants, runs, 3, 2), "plain")
    out["view"]["rays_with_a_live_cell"] = vhit
    for k, b in placements.items():
        out["view"][k].update(batch=batch_stats(b, occ, view, vns[k], 5, vhit))

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
