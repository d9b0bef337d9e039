"""Timing of the distortion loss -> profiles/distortion_timing.json.

  * GraphedTrainStep at 4096 rays x 64 samples and GraphedGuidedTrainStep at 4096 x (64 + 128) (bf16 storage, counter-RNG
    jitter), each without and with the term.  The yardstick is the step without it in the same process -- its launches are
    the ones it had before the term existed.
  * nerf_amd_distortion_loss alone at 640,000 rays x 192 samples (both outputs), beside the compositor's forward on the same
    rays (nerf_amd_volume_render_rays writing w) as a scale.

Variants ALTERNATE in one process; every round times a run of replays (or launches) of each variant between two device events
after a warm-up of every shape, and the figure reported per variant is the median of the rounds (default 5), with the
spread.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from nerf_simple_amd import _lib                                                    # noqa: E402
from nerf_simple_amd.optim import FusedAdam                                         # noqa: E402
from nerf_simple_amd.training import GraphedGuidedTrainStep, GraphedTrainStep       # noqa: E402
from nerf_simple_amd.utils import synthetic                                         # noqa: E402
from nerf_simple_amd.utils.proposal import ProposalVolume                           # noqa: E402
from nerf_simple_amd.utils.xyz import camera_rays, spherical_to_pose               # noqa: E402
from time_background import alternate, fresh                                        # noqa: E402

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--guided", type=int, nargs=2, default=[64, 128], metavar=("Nc", "Nf"))
    ap.add_argument("--stage", type=int, nargs=2, default=[640000, 192], metavar=("B", "N"))
    ap.add_argument("--weight", type=float, default=0.01, help="lambda of the variants with the term")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200, help="replays per round and variant")
    ap.add_argument("--launches", type=int, default=20, help="stage launches per round and variant")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_distortion.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    B, N = a.rays, a.N
    Nc, Nf = a.guided
    gen = torch.Generator().manual_seed(0)
    pose = torch.from_numpy(spherical_to_pose(4, -30, 20)).float()
    side = int(B ** 0.5)
    assert side * side == B, "--rays must be a square number (one small view's rays)"
    rays = camera_rays([pose], [side, side, synthetic.focal_from_fov(side)]).float().contiguous().to(dev)
    gt = torch.rand(B, 3, generator=gen).to(dev)

    def dense(lam):
        net = fresh(dev)
        return GraphedTrainStep(net, FusedAdam(net, lr=5e-4), B, N, device_rng=True, seed=7, check_every=0, distortion=lam)

    prop = ProposalVolume(65, BOUNDS, device=dev)
    prop.update(fresh(dev))

    def guided(lam):
        net = fresh(dev)
        return GraphedGuidedTrainStep(net, FusedAdam(net, lr=5e-4), B, Nc, Nf, prop, device_rng=True, seed=7, check_every=0,
                                      distortion=lam)

    out = dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds, weight=a.weight)
    for name, make, shape in (("train_step", dense, dict(rays=B, N=N)), ("guided_step", guided, dict(rays=B, Nc=Nc, Nf=Nf))):
        steppers = {"plain": make(0.0), "distortion": make(a.weight)}
        res = alternate({k: (lambda s=s: s.step(rays, gt)) for k, s in steppers.items()}, a.rounds, a.steps, 20, dev)
        for k, s in steppers.items():
            res[k]["final_loss"] = float(s.loss)
        res["distortion"]["final_term"] = float(steppers["distortion"].distortion)
        out[name] = dict(**shape, replays_per_round=a.steps, variants=res,
                         over_plain=res["distortion"]["median_ms"] / res["plain"]["median_ms"] - 1.0,
                         extra_ms=res["distortion"]["median_ms"] - res["plain"]["median_ms"])
        for k, v in res.items():
            print(f"{name} {shape}  {k:10s} median {v['median_ms']:.4f} ms  [{v['min_ms']:.4f}, {v['max_ms']:.4f}]")
        del steppers

    # the stage alone, beside the compositor's forward on the same rays
    Bs, Ns = a.stage
    lib, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    raw = torch.randn(Bs, Ns, 4, device=dev)
    ts = torch.sort(torch.rand(Bs, Ns, device=dev) * 4 + 2, dim=1).values.contiguous()
    big = torch.randn(Bs, 6, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    rgb, disp, acc, w = torch.empty(Bs, 3, **f32), torch.empty(Bs, **f32), torch.empty(Bs, **f32), torch.empty(Bs, Ns, **f32)
    loss_ray, g_w = torch.empty(Bs, **f32), torch.empty(Bs, Ns, **f32)

    def render():
        _lib.check(lib.nerf_amd_volume_render_rays(ptr(raw), ptr(ts), ptr(big), ptr(rgb), ptr(disp), None, ptr(acc), ptr(w), Bs, Ns, st),
                   "nerf_amd_volume_render_rays")

    def stage():
        _lib.check(lib.nerf_amd_distortion_loss(ptr(ts), ptr(w), 6.0, 0.25 / Bs, ptr(loss_ray), ptr(g_w), Bs, Ns, st),
                   "nerf_amd_distortion_loss")

    render()
    res = alternate({"volume_render_rays": render, "distortion_loss": stage}, a.rounds, a.launches, 3, dev)
    moved = Bs * Ns * 4 * 3 + Bs * 4                                   # ts and w read, g_w written, loss_ray written
    res["distortion_loss"]["bytes"] = moved
    res["distortion_loss"]["tb_per_s"] = moved / (res["distortion_loss"]["median_ms"] * 1e-3) / 1e12
    out["stage"] = dict(rays=Bs, N=Ns, launches_per_round=a.launches, variants=res)
    for k, v in res.items():
        print(f"stage {Bs} x {Ns}  {k:20s} median {v['median_ms']:.4f} ms  [{v['min_ms']:.4f}, {v['max_ms']:.4f}]")

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
