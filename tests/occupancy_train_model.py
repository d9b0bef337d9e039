"""torch / numpy restatement of training with the occupancy grid (include/nerf_amd.h; csrc/occupancy_train.hip;
utils/occupancy.TrainingOccupancyGrid; training.render_nerf_masked), after tests/occupancy_model.py and
tests/input_grad_model.py.  Test infrastructure; nothing here is fitted to what the GPU showed.

  masked loss: the network is evaluated at the live samples only, its output raw_live [P', 4] is scattered into a dense
      [B, N, 4] tensor whose dead rows are the constants (0, 0, 0, -inf), and the oracle's volume_render composites all N
      samples.  Autograd through that is the definition of every gradient of the masked path.
  decay-max: state <- max(fl32(state * decay), softplus(sigma_now)) in float32 (softplus: beta = 1, identity above 20),
      NaN on either side kept; the bits are occupancy_model.cells_from_density(state, softplus(level), dilate).
  the analytic scene of the end-to-end test: a ball of radius 0.75 with a smooth colour field.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import input_grad_model as IG
import nerf_oracle as O
import occupancy_model as M
from error_model import FACTOR_32, ULP_FLOOR

F32 = np.float32
DEAD_ROW = (0.0, 0.0, 0.0, -np.inf)


# ---- the masked loss ----------------------------------------------------------------------------------------------------
def scatter_live(raw_live, live):
    """raw_live [P', 4] -> dense [B, N, 4] with DEAD_ROW at the dead samples (differentiable in raw_live)."""
    live = torch.from_numpy(np.asarray(live, dtype=bool))
    dense = torch.tensor(DEAD_ROW, dtype=raw_live.dtype).expand(*live.shape, 4).clone()
    dense[live] = raw_live
    return dense


def masked_outputs(raw_live, ts, dn, live):
    return O.volume_render(scatter_live(raw_live, live), ts.to(raw_live.dtype), dn.to(raw_live.dtype))


def geometry(rays, u=None, ts=None):
    """(ts [B,N], query points [B,N,6], unit-direction table) of the oracle, float32 like the kernels' inputs"""
    if ts is None:
        ts = O.sample_ts(u)
    q, dn = O.query_points(rays, ts)
    return ts, q.reshape(rays.shape[0], ts.shape[1], 6), dn


def live_of(q, cells, R, bounds, outside):
    lo, _, inv = M.grid_axes(R, bounds)
    return M.sample_live(q[..., :3].numpy(), cells, lo, inv, outside)


def masked_loss(forward, sd, q, ts, dn, live, gt, dtype):
    """MSE(rgb, gt) of the masked render through ``forward(sd, points)``, in ``dtype``"""
    idx = torch.from_numpy(np.asarray(live, dtype=bool))
    pts = q[idx].to(dtype)
    raw_live = forward(sd, pts) if pts.shape[0] else torch.zeros((0, 4), dtype=dtype) + 0 * sum(t.sum() for t in sd.values())
    rgb = masked_outputs(raw_live, ts.to(dtype), dn.to(dtype), live)[0]
    return F.mse_loss(rgb, gt.to(dtype))


def param_grads(loss_of, forward, sd, dtype):
    sdp = {k: p.detach().to(dtype).requires_grad_(True) for k, p in sd.items()}
    loss = loss_of(forward, sdp, dtype)
    loss.backward()
    return float(loss.detach()), {k: (p.grad.detach() if p.grad is not None else torch.zeros_like(p)) for k, p in sdp.items()}


def model_bound_report(sd, loss_of, grads):
    """The project's rule for the parameter gradients (input_grad_model.bound_bf16, as tests/test_gpu_training.py applies it):
    per tensor, against the float64 masked gradient, the GPU may sit FACTOR_16 x as far as the CPU emulation of the
    kernels' stated roundings (bf16 operands and stored dY, d_raw rounded to bf16 where it enters the chain and the head
    products), with the fp32 oracle's own distance as the floor.  Returns (float64 loss, {tensor: (err, bound)})."""
    loss64, g64 = param_grads(loss_of, IG.exact_forward, sd, torch.float64)
    _, g32 = param_grads(loss_of, IG.exact_forward, sd, torch.float32)
    _, g16 = param_grads(loss_of, functools.partial(IG.emulated_forward, train_heads=True), sd, torch.float32)
    return loss64, {k: (IG.rel_err(grads[k], g64[k]), IG.bound_bf16(g16[k], g32[k], g64[k])) for k in g64}


def central_differences(f, x, idx, h):
    """d f / d x[idx] by central differences (x float64, flat indices)"""
    out = []
    for i in idx:
        xp, xm = x.clone().reshape(-1), x.clone().reshape(-1)
        xp[i] += h
        xm[i] -= h
        out.append((float(f(xp.reshape(x.shape))) - float(f(xm.reshape(x.shape)))) / (2 * h))
    return np.asarray(out)


# ---- the running density volume -----------------------------------------------------------------------------------------
def softplus32(x):
    """the compositor's softplus in numpy float32: identity above 20, log1p(exp(x)) below"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(x > F32(20), x, np.log1p(np.exp(x, dtype=F32), dtype=F32)).astype(F32)


def softplus64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(x > 20, x, np.log1p(np.exp(x)))


def decay_max(state, sigma_now, decay):
    """float32: max(fl(state * decay), softplus(sigma_now)); np.maximum keeps a NaN of either side"""
    with np.errstate(invalid="ignore"):
        return np.maximum((np.asarray(state, F32) * F32(decay)).astype(F32), softplus32(sigma_now)).astype(F32)


def decay_max64(state, sigma_now, decay):
    """the same in float64 on the float32 inputs (the decay product of float32 numbers by the float32 decay)"""
    with np.errstate(invalid="ignore"):
        return np.maximum(np.asarray(state, F32).astype(np.float64) * np.float64(F32(decay)), softplus64(sigma_now))


def decay_max_bound(state, sigma_now, decay):
    """The fp32 rule of tests/error_model.py for the inexact part: FACTOR_32 x numpy-fp32's own distance from the float64
    value + ULP_FLOOR, relative to the largest float64 magnitude (max norm)."""
    want = decay_max64(state, sigma_now, decay)
    scale = float(np.nanmax(np.abs(want)))
    e32 = float(np.nanmax(np.abs(decay_max(state, sigma_now, decay).astype(np.float64) - want))) / scale
    return want, scale, FACTOR_32 * e32 + ULP_FLOOR


def cells_from_state(state, level, dilate):
    """bits of a training grid: the corner / dilation rule on the state volume against softplus(level)"""
    return M.cells_from_density(state, float(softplus32(level)), dilate)


def steps_until_dead(s0, decay, level):
    """the first k >= 1 with decay^k s0 <= softplus(level), the product applied k times in float32 (a cell whose density
    fell to nothing dies at that update)"""
    thr, s, k = softplus32(level), F32(s0), 0
    while True:
        k += 1
        s = F32(s * F32(decay))
        if s <= thr:
            return k
        assert k < 10000


# ---- the analytic scene of the end-to-end test ----------------------------------------------------------------------------
BALL_RADIUS = 0.75
SIGMA_IN, SIGMA_OUT = 8.0, -40.0       # raw sigma: softplus(8) ~ 8 per unit length inside; outside softplus(-40) ~ 4e-18, which
                                       # stays transparent even at the last sample, whose delta is 1e10


def scene_raw(q):
    """raw (r, g, b, sigma) of the analytic ball at query points q [..., 6] (colour: a smooth function of position)"""
    x = q[..., :3]
    inside = (x * x).sum(-1) <= BALL_RADIUS ** 2
    rgb = 0.5 + 0.4 * torch.stack([torch.sin(2.0 * x[..., 0] + 0.3), torch.cos(1.5 * x[..., 1] - 0.2),
                                   torch.sin(1.7 * x[..., 2] + 1.0)], -1)
    sigma = torch.where(inside, torch.full_like(x[..., 0], SIGMA_IN), torch.full_like(x[..., 0], SIGMA_OUT))
    return torch.cat([rgb, sigma[..., None]], -1)


def scene_targets(rays, n_samples=256):
    """the scene composited by the oracle's volume_render at n_samples uniform samples (bin centres) of t in [2, 6]"""
    u = torch.full((rays.shape[0], n_samples), 0.5)
    ts, q, dn = geometry(rays, u=u)
    return O.volume_render(scene_raw(q), ts, dn)[0]
