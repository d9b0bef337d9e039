"""Timing of the image metrics -> profiles/metrics_timing.json.

  * ``image_metrics`` at 800 x 800 on a stride-4 prediction (a view's pixels) against a stride-3 ground truth, M = 1 and
    M = 8 images, with and without SSIM (both launches, the workspace allocation and the double arithmetic behind them).
  * A torch expression of the same SSIM on the device -- separable ``F.conv2d`` blurs, the uncentred form everybody writes --
    plus the squared error: what a user would otherwise write.  Its numbers are not the kernel's (it cancels on flat
    images); only its time is compared.
  * ``render_view`` at 800 x 800 x 128, fp16, device RNG, in the same process: the thing the metrics stand beside.

Variants ALTERNATE in one process; every round times a run of calls of each variant between two device events after a
warm-up of every shape, and the figure reported per variant is the median of the rounds (default 5), with the spread.
Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from nerf_simple_amd.utils import synthetic                                         # noqa: E402
from nerf_simple_amd.utils.metrics import image_metrics                            # noqa: E402
from nerf_simple_amd.utils.nets import Nerf                                         # noqa: E402
from nerf_simple_amd.utils.rendering import render_view                             # noqa: E402
from nerf_simple_amd.utils.xyz import spherical_to_pose                             # noqa: E402
from time_background import timed                                                   # noqa: E402

HBM_BYTES_PER_S = 8.0e12               # MI355X peak, for the byte-time column


def torch_ssim(pred, gt, M, H, W, g):
    """The usual device expression: separable blurs of a, b, a^2, b^2, a b; per image and channel the mean of the map."""
    a = pred.view(M, H, W, -1)[..., :3].permute(0, 3, 1, 2).reshape(M * 3, 1, H, W)
    b = gt.view(M, H, W, -1)[..., :3].permute(0, 3, 1, 2).reshape(M * 3, 1, H, W)

    def blur(x):
        return F.conv2d(F.conv2d(x, g.view(1, 1, 11, 1)), g.view(1, 1, 1, 11))

    mu_a, mu_b = blur(a), blur(b)
    s_aa, s_bb, s_ab = blur(a * a) - mu_a * mu_a, blur(b * b) - mu_b * mu_b, blur(a * b) - mu_a * mu_b
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim = ((2 * mu_a * mu_b + c1) * (2 * s_ab + c2) / ((mu_a * mu_a + mu_b * mu_b + c1) * (s_aa + s_bb + c2))).mean((1, 2, 3))
    sse = ((a - b) ** 2).double().sum((1, 2, 3))
    return ssim.view(M, 3), sse.view(M, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--images", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="metric calls per round and variant")
    ap.add_argument("--renders", type=int, default=3, help="renders per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_metrics.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    S, HW = a.side, a.side * a.side
    gen = torch.Generator().manual_seed(0)
    k = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-(k - 5) ** 2 / 4.5)
    g = (g / g.sum()).float().to(dev)

    net = Nerf(precision="fp16").to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, "structured"))
    cam = [S, S, synthetic.focal_from_fov(S)]
    pose = torch.from_numpy(spherical_to_pose(4, -30, 20)).float()

    def render():
        with torch.no_grad():
            return render_view(net, pose, cam, N=a.N, device_rng=True)

    variants = {"render_view": render}
    data = {}
    for M in a.images:
        pred = torch.rand(M * HW, 4, generator=gen).to(dev)          # a view's pixels: rgb + disparity
        gt = torch.rand(M * HW, 3, generator=gen).to(dev)
        data[M] = (pred, gt)
        variants[f"image_metrics M={M}"] = lambda p=pred, t=gt: image_metrics(p, t, S, S)
        variants[f"image_metrics M={M}, no ssim"] = lambda p=pred, t=gt: image_metrics(p, t, S, S, ssim=False)
        variants[f"torch F.conv2d M={M}"] = lambda p=pred, t=gt, m=M: torch_ssim(p, t, m, S, S, g)
    # a warm-up of every shape; the render is long and gets its own count per round
    for name, fn in variants.items():
        for _ in range(1 if name == "render_view" else 3):
            fn()
    torch.cuda.synchronize(dev)
    times = {k_: [] for k_ in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, a.renders if name == "render_view" else a.calls, dev))
    res = {k_: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds_ms=v) for k_, v in times.items()}

    # how far the torch expression is from the kernel on these (noise) images, for the record
    m1 = image_metrics(*data[a.images[0]], S, S)
    t_ssim, t_sse = torch_ssim(*data[a.images[0]], a.images[0], S, S, g)
    obligatory = HW * (3 + 3) * 4                                    # rgb of both images once; stride 4 moves whole lines: 28 B / pixel
    moved = HW * (4 + 3) * 4
    out = dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds, side=S, N=a.N, calls_per_round=a.calls,
               renders_per_round=a.renders, variants=res,
               bytes_per_pair=dict(rgb_only=obligatory, lines_touched=moved, hbm_byte_time_us=moved / HBM_BYTES_PER_S * 1e6),
               torch_vs_kernel=dict(max_abs_ssim_difference=float((t_ssim.double() - m1.ssim_rgb).abs().max()),
                                    max_rel_sse_difference=float(((t_sse - m1.sse) / m1.sse).abs().max())))
    r = res["render_view"]["median_ms"]
    for name, v in res.items():
        print(f"{name:32s} median {v['median_ms']:9.4f} ms  [{v['min_ms']:.4f}, {v['max_ms']:.4f}]  {100 * v['median_ms'] / r:6.2f} % of a render")
    out["fraction_of_render"] = {name: v["median_ms"] / r for name, v in res.items()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
