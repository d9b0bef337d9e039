"""Time the graphed training step with a per-image colour correction against the plain graphed step, and the five appearance
kernels alone, on one GPU (profiles/appearance_timing.json).

At 4096 rays x 64 samples, bf16, device RNG, a table of 100 images of 400 x 400 (cameras on a ring at radius 4), t in [2, 6],
structured synthetic weights, learning rates 0 so that every step does the same work on the same weights:

  * graphed_plain            -- training.GraphedTrainStep(rays_from=rg);
  * graphed_appearance       -- training.GraphedAppearanceTrainStep, the reduction behind the dX chain (the default);
  * graphed_appearance/head  -- the same with the reduction right behind the head, in front of the fork;
  * gather, apply, apply_backward, reduce and the affine head alone, through the C ABI, at B = 4096 with M = 100 and M = 2000
    images (the plain head beside the affine one).
All variants live in ONE process and are ALTERNATED round by round; a sample is the HIP-event time of `inner` back-to-back
launches after a warm-up, the reported figure the median over the rounds (5), and the spread (max - min over the rounds, relative
to the median) is recorded beside it.

usage: python tools/time_appearance.py [--out profiles/appearance_timing.json] [--rounds 5]     (GPU box)
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
from nerf_simple_amd.training import GraphedAppearanceTrainStep, GraphedTrainStep  # noqa: E402
from nerf_simple_amd.utils import synthetic  # noqa: E402
from nerf_simple_amd.utils.appearance import AppearanceCorrection  # noqa: E402
from nerf_simple_amd.utils.dataload import RayGenerator  # noqa: E402
from nerf_simple_amd.utils.nets import Nerf  # noqa: E402
from nerf_simple_amd.utils.rendering import generate_rays  # noqa: E402
from nerf_simple_amd.utils.xyz import spherical_to_pose  # noqa: E402


class _ReduceBehindHead(GraphedAppearanceTrainStep):
    _reduce_behind = "head"


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
        out[k] = {"median_ms": round(med, 5), "spread": round((max(v) - min(v)) / med, 4), "samples_ms": [round(x, 5) for x in v]}
    return out


def new_net(dev):
    net = Nerf(precision="bf16").to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, "structured"))
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "appearance_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 rounds"
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    B, N, M, side, seed = 4096, 64, 100, 400, 0
    HW = side * side
    cam = [side, side, synthetic.focal_from_fov(side)]
    table = torch.cat([generate_rays(torch.from_numpy(np.asarray(spherical_to_pose(4, -30, 360.0 * m / M), dtype=np.float32)), cam, dev)
                       for m in range(M)])
    colours = torch.rand(M * HW, 3, device=dev)
    rg = RayGenerator.from_tables(table, colours)
    res = {"device": torch.cuda.get_device_name(0), "step": {"rays": B, "N": N, "images": M, "image": [side, side], "precision": "bf16"},
           "rounds": args.rounds, "inner_launches_per_sample": args.inner}

    # ---- the steppers ----
    steppers = {}
    net = new_net(dev)
    steppers["graphed_plain"] = GraphedTrainStep(net, FusedAdam(net, lr=0.0), B, N, rays_from=rg, device_rng=True, seed=seed, check_every=0)
    for name, cls in (("graphed_appearance", GraphedAppearanceTrainStep), ("graphed_appearance/head", _ReduceBehindHead)):
        net = new_net(dev)
        app = AppearanceCorrection(M, HW, dev, reg=1e-3, frozen=(0,))
        steppers[name] = cls(net, FusedAdam(net, lr=0.0), B, N, app, rays_from=rg, appearance_lr=0.0, device_rng=True, seed=seed,
                             check_every=0)
    timed = alternated({k: s.step for k, s in steppers.items()}, args.rounds, args.inner)
    plain = timed["graphed_plain"]["median_ms"]
    res["steps"] = timed
    for k in ("graphed_appearance", "graphed_appearance/head"):
        d = timed[k]["median_ms"] - plain
        timed[k]["minus_plain_ms"] = round(d, 5)
        timed[k]["difference_exceeds_the_spread"] = bool(abs(d) > max(timed[k]["spread"], timed["graphed_plain"]["spread"]) * plain)

    # ---- the five kernels alone ----
    st = _lib.stream_ptr(dev)
    ptr = _lib.ptr
    f32 = dict(dtype=torch.float32, device=dev)
    s = steppers["graphed_appearance"]             # raw / ts / rays / gt of a real step
    res["kernels"] = {}
    for M_k, HW_k in ((100, HW), (2000, HW // 20)):
        theta = torch.randn(M_k, 6, **f32) * 0.1
        ids = torch.randint(0, M_k * HW_k, (B,), dtype=torch.int64, device=dev)
        kept, rows, g_ray = torch.empty_like(ids), torch.empty((B, 6), **f32), torch.empty((B, 6), **f32)
        out, g_rgb, g_theta = torch.empty((B, 3), **f32), torch.empty((B, 3), **f32), torch.empty((M_k, 6), **f32)
        rgb, d_raw = torch.empty((B, 3), **f32), torch.empty_like(s.d_raw)
        frozen = torch.zeros(M_k, dtype=torch.int32, device=dev)
        lib.nerf_amd_appearance_gather(ptr(theta), ptr(ids), ptr(kept), HW_k, ptr(rows), B, M_k, st)
        kern = {
            "gather": lambda: lib.nerf_amd_appearance_gather(ptr(theta), ptr(ids), ptr(kept), HW_k, ptr(rows), B, M_k, st),
            "apply": lambda: lib.nerf_amd_appearance_apply(ptr(s.rgb), ptr(rows), 6, ptr(out), B, st),
            "apply_backward": lambda: lib.nerf_amd_appearance_apply_backward(ptr(out), ptr(s.rgb), ptr(rows), 6, ptr(g_rgb), ptr(g_ray), B, st),
            "reduce": lambda: lib.nerf_amd_appearance_reduce(ptr(g_ray), ptr(ids), HW_k, ptr(theta), 1e-3, ptr(frozen), ptr(g_theta), B, M_k, st),
            "affine_head": lambda: lib.nerf_amd_volume_render_mse_backward_affine(ptr(s.raw), ptr(s.ts), ptr(s.rays), ptr(s.gt), ptr(rows), 6,
                                                                                  ptr(rgb), ptr(g_ray), ptr(d_raw), B, N, st),
            "plain_head": lambda: lib.nerf_amd_volume_render_mse_backward(ptr(s.raw), ptr(s.ts), ptr(s.rays), ptr(s.gt), ptr(rgb),
                                                                          ptr(d_raw), B, N, st),
        }
        k = alternated(kern, args.rounds, 50)
        res["kernels"][f"B{B}_M{M_k}"] = {n: {"median_ms": v["median_ms"], "spread": v["spread"]} for n, v in k.items()}
    res["largest_step_spread"] = max(v["spread"] for v in timed.values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"steps": {k: {"median_ms": v["median_ms"], "spread": v["spread"], "minus_plain_ms": v.get("minus_plain_ms")}
                                for k, v in timed.items()}, "kernels": res["kernels"]}))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
