"""Timing of the input gradients (csrc/input_grad.hip) by HIP events, at the training workload's size
(4096 rays x 64 samples = 262,144 points), bf16, structured synthetic weights:

  kernel     nerf_amd_input_gradients in rays mode alone (the products, the encoder Jacobian, the ray reduction),
             on the dY of one nerf_amd_mlp_backward; its HBM bytes (dY0 | dY5 | dY9 read, 1280 B / point, plus the
             per-sample gradient written and re-read and the rays / ts) against the time those bytes take at 6 TB/s;
  pose step  render_nerf + MSE + backward with a FROZEN net and rays requiring grad: forward, compositor backward,
             dX chain and input gradient, no dW (what a pose-estimation step pays);
  train step the same call with a trainable net and rays not requiring grad (the existing bf16 training step's
             forward / backward, dW included), for comparison on the same box.

    python tools/time_input_grad.py [out.json]     (writes one JSON object; prints it too)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_simple_amd import _lib                                   # noqa: E402
from nerf_simple_amd.utils import synthetic                        # noqa: E402
from nerf_simple_amd.utils.nets import Nerf                        # noqa: E402
from nerf_simple_amd.utils.rendering import render_nerf            # noqa: E402
from nerf_simple_amd.utils.xyz import camera_rays, spherical_to_pose   # noqa: E402

HBM_BYTES_PER_S = 6e12


def timed(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us


def main():
    dev = torch.device("cuda:0")
    B, N = 4096, 64
    P = B * N
    sd = synthetic.synthetic_state_dict(0, "structured")
    net = Nerf(precision="bf16").to(dev)
    net.load_state_dict(sd)
    pose = torch.from_numpy(spherical_to_pose(4, -30, 0)).float()
    rays = camera_rays([pose], [64, 64, synthetic.focal_from_fov(64)]).to(dev).contiguous()
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(0)).to(dev)
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    lib = _lib.lib()
    st = _lib.stream_ptr(dev)

    # one training forward + dX chain to get a real dY
    tbins = torch.linspace(2, 6, N + 1).to(dev)
    acts = torch.empty(int(lib.nerf_amd_train_activation_bytes(P)), dtype=torch.uint8, device=dev)
    raw = torch.empty(B, N, 4, device=dev)
    ts = torch.empty(B, N, device=dev)
    _lib.check(lib.nerf_amd_mlp_forward_train(_lib.ptr(rays), _lib.ptr(u), _lib.ptr(tbins), _lib.ptr(net.packed_weights(_lib.BF16)),
                                              0, 0, 0, _lib.ptr(raw), _lib.ptr(ts), _lib.ptr(acts), B, N, st), "forward_train")
    g = torch.randn(P, 4, generator=torch.Generator().manual_seed(2)).to(dev) * 1e-3
    dys = torch.empty_like(acts)
    _lib.check(lib.nerf_amd_mlp_backward(_lib.ptr(g), _lib.ptr(net.packed_weights(_lib.BF16_BWD)), _lib.ptr(acts), _lib.ptr(dys),
                                         P, st), "mlp_backward")
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    dv = torch.empty(P, 6, device=dev)
    d_rays = torch.empty(B, 6, device=dev)

    def kernel():
        _lib.check(lib.nerf_amd_input_gradients(_lib.ptr(dys), _lib.ptr(flat), None, _lib.ptr(rays), _lib.ptr(ts), _lib.ptr(dv),
                                                _lib.ptr(d_rays), P, N, st), "input_gradients")

    def step(frozen):
        net.requires_grad_(not frozen)
        r = rays.clone().requires_grad_(frozen)

        def run():
            net.zero_grad(set_to_none=True)
            loss = torch.nn.functional.mse_loss(render_nerf(r, net, N, u=u)[0], target)
            loss.backward()
        return run

    k_us = timed(kernel, reps=200)
    nbytes = P * (1280 + 24 + 24 + 4) + B * 48
    out = {
        "points": P, "rays": B, "N": N,
        "input_gradient_kernel_us": round(k_us, 1),
        "input_gradient_bytes": nbytes,
        "input_gradient_byte_time_us_at_6TBps": round(nbytes / HBM_BYTES_PER_S * 1e6, 1),
        "input_gradient_achieved_TBps": round(nbytes / (k_us * 1e-6) / 1e12, 2),
        "pose_step_frozen_net_us": round(timed(step(True)), 1),
        "train_step_bf16_us": round(timed(step(False)), 1),
        "device": torch.cuda.get_device_name(dev),
    }
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
