"""Timing of the camera optimiser -> profiles/camera_timing.json.

  * GraphedTrainStep(rays_from=rg) and GraphedCameraTrainStep at 4096 rays x 64 samples (bf16 storage, counter-RNG jitter,
    the selection inside the graph) on a table of 100 images of 400 x 400.  The yardstick is the plain step in the same
    process -- its launches are the ones it had before the cameras existed.
  * nerf_amd_camera_rays, nerf_amd_camera_rays_backward and nerf_amd_camera_poses, each alone at B = 4096 with
    M in {100, 2000} images of 400 x 400 (ids drawn uniformly over the table; no table is needed for them).

Variants ALTERNATE in one process; every round times a run of replays (or launches) of each variant between two device events
after a warm-up of every shape, and the figure reported per variant is the median of the rounds (default 5), with the
spread.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from nerf_simple_amd import _lib                                                    # noqa: E402
from nerf_simple_amd.optim import FusedAdam                                         # noqa: E402
from nerf_simple_amd.training import GraphedCameraTrainStep, GraphedTrainStep       # noqa: E402
from nerf_simple_amd.utils import synthetic                                         # noqa: E402
from nerf_simple_amd.utils.cameras import CameraRefinement                          # noqa: E402
from nerf_simple_amd.utils.dataload import RayGenerator                             # noqa: E402
from nerf_simple_amd.utils.xyz import spherical_to_pose                             # noqa: E402
from time_background import alternate, fresh                                        # noqa: E402


def poses_on_a_sphere(M):
    return torch.stack([torch.from_numpy(spherical_to_pose(4, -20 - 40 * (m % 7) / 7, 360.0 * m / M)).float() for m in range(M)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--side", type=int, default=400)
    ap.add_argument("--kernel-images", type=int, nargs="+", default=[100, 2000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200, help="replays per round and variant")
    ap.add_argument("--launches", type=int, default=200, help="kernel launches per round and variant")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_camera.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    B, N, M, S = a.rays, a.N, a.images, a.side
    cam = [S, S, synthetic.focal_from_fov(S)]
    gen = np.random.default_rng(0)
    samples = {"train": [{"img": gen.random((S, S, 3), dtype=np.float32), "transform": p.numpy()} for p in poses_on_a_sphere(M)]}
    rg = RayGenerator.from_samples(samples, cam, dev)
    del samples

    def plain():
        net = fresh(dev)
        return GraphedTrainStep(net, FusedAdam(net, lr=5e-4), B, N, rays_from=rg, device_rng=True, seed=7, check_every=0)

    def camera():
        net = fresh(dev)
        return GraphedCameraTrainStep(net, FusedAdam(net, lr=5e-4), B, N, CameraRefinement.from_ray_generator(rg), rays_from=rg,
                                      camera_lr=1e-3, device_rng=True, seed=7, check_every=0)

    out = dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds)
    steppers = {"plain": plain(), "camera": camera()}
    res = alternate({k: s.step for k, s in steppers.items()}, a.rounds, a.steps, 20, dev)
    for k, s in steppers.items():
        res[k]["final_loss"] = float(s.loss)
    res["camera"]["final_xi_max"] = float(steppers["camera"].cameras.xi.detach().abs().max())
    out["train_step"] = dict(rays=B, N=N, images=M, side=S, replays_per_round=a.steps, variants=res,
                             over_plain=res["camera"]["median_ms"] / res["plain"]["median_ms"] - 1.0,
                             extra_ms=res["camera"]["median_ms"] - res["plain"]["median_ms"])
    for k, v in res.items():
        print(f"train_step {B} x {N}, {M} images of {S} x {S}  {k:8s} median {v['median_ms']:.4f} ms  [{v['min_ms']:.4f}, {v['max_ms']:.4f}]")
    del steppers, rg

    # the three kernels alone
    lib, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    out["kernels"] = {}
    for Mk in a.kernel_images:
        g = torch.Generator().manual_seed(Mk)
        poses0 = poses_on_a_sphere(Mk)[:, :3].contiguous().to(dev)
        xi = (0.01 * torch.randn(Mk, 6, generator=g)).to(dev)
        ids = torch.randint(0, Mk * S * S, (B,), generator=g).to(dev)
        d_rays = torch.randn(B, 6, generator=g).to(dev)
        rays, kept = torch.empty(B, 6, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
        g_xi, top = torch.empty(Mk, 6, device=dev), torch.empty(Mk, 3, 4, device=dev)

        def k_rays():
            _lib.check(lib.nerf_amd_camera_rays(ptr(poses0), ptr(xi), ptr(ids), ptr(kept), S, S, cam[2], ptr(rays), B, Mk, st),
                       "nerf_amd_camera_rays")

        def k_backward():
            _lib.check(lib.nerf_amd_camera_rays_backward(ptr(poses0), ptr(xi), ptr(ids), ptr(d_rays), S, S, cam[2], ptr(g_xi), None,
                                                         B, Mk, st), "nerf_amd_camera_rays_backward")

        def k_poses():
            _lib.check(lib.nerf_amd_camera_poses(ptr(poses0), ptr(xi), ptr(top), Mk, st), "nerf_amd_camera_poses")

        res = alternate({"camera_rays": k_rays, "camera_rays_backward": k_backward, "camera_poses": k_poses}, a.rounds, a.launches,
                        10, dev)
        out["kernels"][f"M{Mk}"] = dict(rays=B, images=Mk, side=S, launches_per_round=a.launches, variants=res)
        for k, v in res.items():
            print(f"B = {B}, M = {Mk}  {k:22s} median {v['median_ms'] * 1e3:.2f} us  [{v['min_ms'] * 1e3:.2f}, {v['max_ms'] * 1e3:.2f}]")

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
