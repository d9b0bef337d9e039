"""Yardsticks of the gradients with respect to the INPUTS (query points, rays, camera pose), after tests/error_model.py.

Truth is float64 torch autograd through the oracle (oracle/nerf_oracle.py, pinned to the reference).  Tolerances come
from models of the stated numerics, computed here on the CPU, never from what the GPU showed:

  fp32 paths: the fp32 oracle's own autograd sits e32 = |fp32 - float64| from the truth (max norm over the tensor,
      relative to the tensor's largest float64 magnitude); the GPU is allowed FACTOR_32 x e32 + ULP_FLOOR.
  bf16 paths: an emulation of the kernels' numerics -- the oracle's forward and backward with every layer's weights
      and inputs (encoder features, activations) rounded to bf16, fp32 products and sums, fp32 bias, and every stored
      pre-activation gradient dY rounded to bf16 (gradient hooks on the pre-activations of layers_0.*, skip_conn_layer,
      layers_1.*, layers_2 and color_fc.0 -- what nerf_amd_mlp_backward writes); the encoder's Jacobian, the sampler
      and the compositor in fp32, as in the kernels.  Its distance e16 from the truth is the error the bf16 operands
      cost; the GPU is allowed FACTOR_16 x e16, plus the fp32 bound as a floor.
"""
import math

import torch
import torch.nn.functional as F

import nerf_oracle as O
from error_model import FACTOR_16, FACTOR_32, ULP_FLOOR

# the 10 layers whose pre-activation gradient the dX chain stores in bf16 (csrc/nerf_layout.h: dY0 .. dY9)
DY_LAYERS = ("layers_0.0", "layers_0.2", "layers_0.4", "layers_0.6", "layers_0.8", "skip_conn_layer.0",
             "layers_1.0", "layers_1.2", "layers_2", "color_fc.0")


def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


class _RoundBf16(torch.autograd.Function):
    """bf16 rounding of a forward operand; the gradient passes unchanged (the kernels' dX is fp32 until stored)."""

    @staticmethod
    def forward(ctx, x):
        return _bf16(x)

    @staticmethod
    def backward(ctx, g):
        return g


def _round_dy(y):
    if y.requires_grad:
        y.register_hook(_bf16)
    return y


def emulated_forward(sd, v, Lp=10, Ld=4, train_heads=False):
    """Nerf.forward with the bf16 training kernels' numerics (forward and backward), fp32: [P,6] -> [P,4].

    ``train_heads`` adds the two roundings that only the PARAMETER gradients see (tests/train_chain_model.py): d_raw is
    rounded to bf16 where it enters the dX chain (csrc/mlp_bwd_16.hip bx_rgb / bx_sig) and in the two head products
    (csrc/dw_gemm.hip pack_draw_kernel: sigma_fc.0.weight, color_fc.2.weight); the head biases sum the fp32 d_raw.  The
    input-gradient tests were written against the emulation without it."""
    r = _RoundBf16.apply

    def lin(h, name, dy=True):
        if train_heads and not dy:
            y = _round_dy(F.linear(r(h), r(sd[name + ".weight"])))      # weight and input see bf16(d_raw) ...
            return y + sd[name + ".bias"]                               # ... the bias the fp32 one
        y = F.linear(r(h), r(sd[name + ".weight"]), sd[name + ".bias"])
        return _round_dy(y) if dy else y

    x, d = O.positional_encoder(v, Lp, Ld)
    h = x
    for i in (0, 2, 4, 6, 8):
        h = F.relu(lin(h, f"layers_0.{i}"))
    h = F.relu(lin(torch.cat([h, x], 1), "skip_conn_layer.0"))
    for i in (0, 2):
        h = F.relu(lin(h, f"layers_1.{i}"))
    sigma = lin(h, "sigma_fc.0", dy=False)
    h9 = lin(h, "layers_2")
    c = F.relu(lin(torch.cat([h9, d], 1), "color_fc.0"))
    rgb = lin(c, "color_fc.2", dy=False)
    return torch.cat([rgb, sigma], 1)


def exact_forward(sd, v, Lp=10, Ld=4):
    return O.nerf_forward(sd, v, Lp, Ld)


def cast_sd(sd, dtype):
    return {k: t.to(dtype) for k, t in sd.items()}


def render(forward, sd, rays, N, u=None, ts=None):
    """render_nerf (utils/rendering.py:13-45) through ``forward``: the 5-tuple, differentiable in rays."""
    if ts is None:
        ts = O.sample_ts(u).to(rays.dtype)
    q, dn = O.query_points(rays, ts.to(rays.dtype))
    out = forward(sd, q).reshape(rays.shape[0], N, 4)
    return O.volume_render(out, ts.to(rays.dtype), dn)


def points_grad(forward, sd, v, G, dtype):
    """d sum(forward(v) * G) / d v in ``dtype`` (and d / d parameters, as a dict)."""
    v = v.detach().to(dtype).requires_grad_(True)
    sdp = {k: t.detach().to(dtype).requires_grad_(True) for k, t in sd.items()}
    (forward(sdp, v) * G.to(dtype)).sum().backward()
    return v.grad.detach(), {k: t.grad.detach() for k, t in sdp.items()}


def ray_loss(outs, target):
    return F.mse_loss(outs[0], target.to(outs[0].dtype))


def rays_grad(forward, sd, rays, N, target, dtype, u=None, ts=None):
    """d MSE(rgb, target) / d rays in ``dtype``."""
    rays = rays.detach().to(dtype).requires_grad_(True)
    sdd = cast_sd(sd, dtype)
    ray_loss(render(forward, sdd, rays, N, u=u, ts=ts), target).backward()
    return rays.grad.detach()


def rel_err(got, want):
    """max |got - want| / max |want| (gradients have no natural unit scale)."""
    want = want.double()
    scale = float(want.abs().max())
    return float((got.double().cpu() - want).abs().max()) / max(scale, 1e-300)


def bound_fp32(g32, g64):
    return FACTOR_32 * rel_err(g32, g64) + ULP_FLOOR


def bound_bf16(g16, g32, g64):
    return FACTOR_16 * rel_err(g16, g64) + bound_fp32(g32, g64)


# ---- camera pose as a learnable 6-vector --------------------------------------------------------------
def skew(w):
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def pose_rays(xi, pose0, dirs_cam):
    """xi [6] = (axis-angle w, translation tau) applied to pose0 [4,4]: R = exp([w]x) R0, t = t0 + tau;
    dirs_cam [3, n] camera-frame directions -> world rays [n, 6] (utils/rendering.py:129-134)."""
    R = torch.linalg.matrix_exp(skew(xi[:3])) @ pose0[:3, :3]
    t = pose0[:3, 3] + xi[3:]
    d = (R @ dirs_cam).T
    return torch.cat([t.expand(d.shape[0], 3), d], dim=1)


def pose_error(xi, xi_true):
    """rotation angle (rad) + translation distance of the estimate from the truth."""
    dw = (xi[:3] - xi_true[:3]).double()
    return float(dw.norm()) + float((xi[3:] - xi_true[3:]).double().norm())


def start_perturbation(dtype=torch.float32):
    """about 1 degree about a fixed oblique axis and 0.03 of translation (units of the scene: camera at radius 4)."""
    axis = torch.tensor([0.6, -0.48, 0.64], dtype=torch.float64)
    axis = axis / axis.norm()
    w = axis * math.radians(1.0)
    tau = torch.tensor([0.02, -0.015, 0.0158], dtype=torch.float64)
    return torch.cat([w, tau]).to(dtype)


def smooth_state_dict(sd, max_level=3):
    """``sd`` with the position-encoder columns of levels >= max_level cut from layers_0.0 and the skip layer: a scene
    without the 2^9-per-unit detail of the full encoder, whose photometric loss is smooth enough over a degree of pose
    for a first-order optimiser to descend (a random network at full bandwidth is noise at that scale)."""
    out = {k: t.clone() for k, t in sd.items()}
    cols = [3 + 20 * c + 2 * l + t for c in range(3) for l in range(max_level, 10) for t in range(2)]
    out["layers_0.0.weight"][:, cols] = 0
    out["skip_conn_layer.0.weight"][:, [256 + c for c in cols]] = 0
    return out
