"""Timing of the dense path's two training controls -> profiles/background_timing.json.

  * GraphedTrainStep at 4096 rays x 64 samples (bf16 storage, counter-RNG jitter): plain, background only, noise only, both.
    The yardstick is the plain step in the same process -- its launches are the ones it had before the controls existed.
  * render_view at 800 x 800 x 128 (bf16, counter-RNG jitter) without and with a background: the one-call image render
    against device ray generation + nerf_amd_render_forward (rgb, disp, acc) + the blend launch.

Variants ALTERNATE in one process; every round times a run of replays (or renders) of each variant between two device events
after a warm-up of every shape, and the figure reported per variant is the median of the rounds (default 5), with the
spread.  Needs a GPU: there is no fallback.  Kernel-level numbers come from a rocprofv3 run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/time_background.py --rounds 2
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_simple_amd.optim import FusedAdam                                         # noqa: E402
from nerf_simple_amd.training import GraphedTrainStep                               # noqa: E402
from nerf_simple_amd.utils import synthetic                                         # noqa: E402
from nerf_simple_amd.utils.nets import Nerf                                         # noqa: E402
from nerf_simple_amd.utils.rendering import render_view                             # noqa: E402
from nerf_simple_amd.utils.xyz import camera_rays, spherical_to_pose               # noqa: E402


def fresh(dev):
    net = Nerf(precision="bf16").to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, "default"))
    return net


def timed(fn, reps, dev):
    """Milliseconds per call of ``fn`` over ``reps`` calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / reps


def alternate(variants, rounds, reps, warmup, dev):
    """{name: {"median_ms", "min_ms", "max_ms", "rounds_ms"}}: the variants take turns inside every round."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, reps, dev))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds_ms=v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200, help="replays per round and variant")
    ap.add_argument("--view", type=int, nargs=3, default=[800, 800, 128], metavar=("H", "W", "N"))
    ap.add_argument("--renders", type=int, default=3, help="renders per round and variant")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "background_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_background.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    B, N = a.rays, a.N
    gen = torch.Generator().manual_seed(0)
    pose = torch.from_numpy(spherical_to_pose(4, -30, 20)).float()
    side = int(B ** 0.5)
    assert side * side == B, "--rays must be a square number (one small view's rays)"
    rays = camera_rays([pose], [side, side, synthetic.focal_from_fov(side)]).float().contiguous().to(dev)
    gt = torch.rand(B, 3, generator=gen).to(dev)
    white = torch.ones(3, device=dev)

    controls = {"plain": {}, "background": dict(background=white), "noise": dict(sigma_noise=1.0, noise_seed=11),
                "both": dict(background=white, sigma_noise=1.0, noise_seed=11)}
    steppers = {}
    for name, kw in controls.items():
        net = fresh(dev)
        steppers[name] = GraphedTrainStep(net, FusedAdam(net, lr=5e-4), B, N, device_rng=True, seed=7, check_every=0, **kw)
    step = alternate({k: (lambda s=s: s.step(rays, gt)) for k, s in steppers.items()}, a.rounds, a.steps, 20, dev)
    for k, s in steppers.items():
        step[k]["final_loss"] = float(s.loss)

    H, W, Nv = a.view
    net = fresh(dev)
    cam = [H, W, synthetic.focal_from_fov(W)]
    with torch.no_grad():
        view = alternate({"plain": lambda: render_view(net, pose.numpy(), cam, N=Nv, device_rng=True, seed=5),
                          "background": lambda: render_view(net, pose.numpy(), cam, N=Nv, device_rng=True, seed=5, background=white)},
                         a.rounds, a.renders, 2, dev)

    def rel(d, k):
        return d[k]["median_ms"] / d["plain"]["median_ms"] - 1.0

    out = dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds,
               train_step=dict(rays=B, N=N, replays_per_round=a.steps, variants=step,
                               over_plain={k: rel(step, k) for k in step if k != "plain"}),
               render_view=dict(H=H, W=W, N=Nv, renders_per_round=a.renders, variants=view,
                                over_plain={"background": rel(view, "background")},
                                extra_ms=view["background"]["median_ms"] - view["plain"]["median_ms"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for k, v in step.items():
        print(f"train step {B} x {N}  {k:10s} median {v['median_ms']:.4f} ms  [{v['min_ms']:.4f}, {v['max_ms']:.4f}]")
    for k, v in view.items():
        print(f"render_view {H}x{W}x{Nv}  {k:10s} median {v['median_ms']:.3f} ms  [{v['min_ms']:.3f}, {v['max_ms']:.3f}]")


if __name__ == "__main__":
    main()
