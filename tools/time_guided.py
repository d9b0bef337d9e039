"""Timing of grid-guided fine sampling next to what it stands in for.  All variants of a group run
in ONE process, alternating, and the median of 5 timed runs (HIP events, after warm-up) is reported:

  * sampler:  nerf_amd_sample_pdf_volume at 640,000 rays x (64 + 128) over a 128^3 volume, next to nerf_amd_sample_pdf on
              the same rays (positions and weights read from HBM);
  * render:   render_guided_view against render_hierarchical_view and render_view(N = 192), 800 x 800, fp16, counter RNG;
  * step:     GraphedGuidedTrainStep against GraphedHierarchicalTrainStep and GraphedTrainStep(N = 192) at 4096 rays;
  * update:   ProposalVolume.update at 128^3.

Writes profiles/guided_timing.json.  The baselines are entry points this feature does not touch."""
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
from nerf_simple_amd.training import GraphedGuidedTrainStep, GraphedHierarchicalTrainStep, GraphedTrainStep      # noqa: E402
from nerf_simple_amd.utils import synthetic                                                          # noqa: E402
from nerf_simple_amd.utils.nets import Nerf                                                          # noqa: E402
from nerf_simple_amd.utils.proposal import ProposalVolume                                            # noqa: E402
from nerf_simple_amd.utils.rendering import (generate_rays, render_guided_view, render_hierarchical_view, render_view,      # noqa: E402
                                             sample_pdf)
from nerf_simple_amd.utils.xyz import spherical_to_pose                                              # noqa: E402


def alternate(variants, runs, reps, warmup):
    """{name: median ms per call} of callables timed in alternating order."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--Nc", type=int, default=64)
    ap.add_argument("--Nf", type=int, default=128)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    Nc, Nf, N, runs = args.Nc, args.Nf, args.Nc + args.Nf, args.runs
    net_c, net_f = net_on(dev, 0), net_on(dev, 1)
    prop = ProposalVolume(args.resolution, device=dev)
    out = {"config": {"view": [args.side, args.side], "train_rays": args.rays, "Nc": Nc, "Nf": Nf, "resolution": args.resolution,
                      "runs": runs, "device": torch.cuda.get_device_name(dev)}}

    out["update"] = alternate({"ProposalVolume.update": lambda: prop.update(net_f)}, runs, 10, 3)

    # ---- the sampler alone ----
    pose = spherical_to_pose(4, -30, 0)
    cam = (args.side, args.side, synthetic.focal_from_fov(args.side))
    rays = generate_rays(pose, cam, dev)
    B = rays.shape[0]
    ts, _, w_c = prop.sample(rays, Nc, Nf, device_rng=True, seed=1, return_weights=True)
    ts_c = prop.sample(rays, Nc, 0, device_rng=True, seed=1)              # Nf = 0: the coarse positions themselves
    ts_out = torch.empty_like(ts)
    tbins = torch.linspace(2, 6, Nc + 1).to(dev)

    def guided():
        prop._launch(rays, None, tbins, _lib.FLAG_DEVICE_RNG, 1, 0, None, ts_out, None, None, B, Nc, Nf)

    out["sampler"] = alternate({"nerf_amd_sample_pdf_volume": guided,
                                "nerf_amd_sample_pdf": lambda: sample_pdf(ts_c, w_c, Nf, device_rng=True, seed=1)}, runs, 10, 3)
    out["sampler"]["rays"] = B

    # ---- one view ----
    with torch.no_grad():
        out["render"] = alternate({
            "render_guided_view": lambda: render_guided_view(net_f, pose, cam, Nc, Nf, prop, device_rng=True, precision="fp16"),
            "render_hierarchical_view": lambda: render_hierarchical_view(net_c, net_f, pose, cam, Nc, Nf, device_rng=True,
                                                                         precision="fp16"),
            f"render_view N={N}": lambda: render_view(net_f, pose, cam, N=N, device_rng=True, precision="fp16")}, runs, 3, 2)

    # ---- the graphed training step ----
    g = torch.Generator().manual_seed(0)
    sel = torch.randperm(B, generator=g)[:args.rays].to(dev)
    trays, gt = rays[sel].contiguous(), torch.rand(args.rays, 3, generator=g).to(dev)
    a, b, c, d = (net_on(dev, s, "default") for s in (0, 1, 2, 3))
    tprop = ProposalVolume(args.resolution, device=dev).update(a)
    steppers = {
        "GraphedGuidedTrainStep": GraphedGuidedTrainStep(a, FusedAdam(a, lr=5e-4), args.rays, Nc, Nf, tprop, device_rng=True,
                                                         seed=7, check_every=0),
        "GraphedHierarchicalTrainStep": GraphedHierarchicalTrainStep(b, c, FusedAdam([b, c], lr=5e-4), args.rays, Nc, Nf,
                                                                     device_rng=True, seed=7, check_every=0),
        f"GraphedTrainStep N={N}": GraphedTrainStep(d, FusedAdam(d, lr=5e-4), args.rays, N, device_rng=True, seed=7,
                                                    check_every=0)}
    out["step"] = alternate({k: (lambda s=s: s.step(trays, gt)) for k, s in steppers.items()}, runs, 50, 10)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
