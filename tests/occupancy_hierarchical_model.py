"""torch / numpy restatement of the masked hierarchical pair (include/nerf_amd.h, "masked hierarchical pair";
csrc/occupancy_graph.hip; training.train_step_hierarchical(occupancy=) / GraphedMaskedHierarchicalTrainStep; DESIGN.md
section 15), built from tests/occupancy_model.py, tests/occupancy_train_model.py, tests/occupancy_graphed_model.py and the
oracle's sample_pdf.  Test infrastructure; nothing here is fitted to what the GPU showed.

ONE grid masks both passes.  With ``live_c`` [B, Nc] the grid's verdict on the coarse samples and C_c the coarse capacity:

  coarse pass: the masked render under mask_C(live_c, C_c): the network's rows scattered into a dense [B, Nc, 4] tensor whose
      dead rows are (0, 0, 0, -inf); the oracle's volume_render gives rgb_c and w_c, w_c = 0 exactly at a dead sample.
  sampler:     ts_f = oracle.sample_pdf(ts_c, w_c.detach(), u_f): the coarse positions kept and merged.  A ray with nothing kept
      has w_c == 0, the 1e-5 floor makes its pdf uniform over the interior bins.
  fine pass:   the masked render on ts_f through the same grid under mask_C(live_f, C_f), live_f the grid's verdict on the
      fine samples' positions.
  loss = MSE(rgb_c, gt) + MSE(rgb_f, gt); the coarse network learns from its own term only.
"""
import numpy as np
import torch

import nerf_oracle as O
import occupancy_graphed_model as G
import occupancy_model as M
import occupancy_train_model as T


def pair_inputs(oracle, synthetic, B, Nc, Nf):
    """the rays, targets and coarse jitter of tests/test_gpu_occupancy_graphed.py::step_inputs at (B, Nc), and u_f [B, Nf]"""
    gen = torch.Generator().manual_seed(B * 1000 + Nc)
    pose = torch.from_numpy(oracle.spherical_to_pose(4, -30, 0)).float()
    side = int(np.ceil(np.sqrt(B)))
    rays = oracle.camera_rays(pose, [side, side, synthetic.focal_from_fov(side)])[:B].contiguous()
    gt = torch.rand(B, 3, generator=gen)
    u_c = torch.rand(B, Nc, generator=gen)
    u_f = torch.rand(B, Nf, generator=torch.Generator().manual_seed(B * 1000 + Nc + 7919 * Nf))
    return rays, gt, u_c, u_f


def coarse_head(raw_live, ts_c, dn, live, C, gt, u_f):
    """The masked coarse head under the capacity clamp, by autograd: raw_live [P', 4] (rows behind min(P', C) are never
    looked at) -> (rgb [B, 3], d_raw [C, 4] with zero rows behind the kept ones, ts_f [B, Nc + Nf], w [B, Nc])."""
    kept = G.mask_C(live, C)
    K = int(kept.sum())
    raw = raw_live[:K].detach().clone().requires_grad_(True)
    rgb, _, _, _, w = T.masked_outputs(raw, ts_c, dn, kept)
    loss = torch.nn.functional.mse_loss(rgb, gt.to(rgb.dtype))
    loss.backward()
    d = torch.zeros((int(C), 4), dtype=raw.dtype)
    if K:
        d[:K] = raw.grad
    ts_f = O.sample_pdf(ts_c.to(raw.dtype), w.detach(), u_f.to(raw.dtype))
    return rgb.detach(), d, ts_f, w.detach()


def uniform_rows(ts_c, u_f):
    """what the sampler gives a ray whose weights are all zero: the inverse cdf of the uniform pdf over the interior bins"""
    return O.sample_pdf(ts_c, torch.zeros_like(ts_c), u_f)


def fine_live(rays, ts_f, cells, R, bounds, outside):
    _, q, _ = T.geometry(rays, ts=ts_f)
    return T.live_of(q, cells, R, bounds, outside)


def pair_losses(forward, sd_c, sd_f, rays, u_c, u_f, cells, R, bounds, outside, gt, dtype, C_c=None, C_f=None):
    """(MSE(rgb_c, gt), MSE(rgb_f, gt), live_c, live_f, ts_f) of the masked pair through ``forward(sd, points)`` in ``dtype``;
    capacities None = no clamp."""
    ts_c, q_c, dn = T.geometry(rays, u=u_c)
    live_c = T.live_of(q_c, cells, R, bounds, outside)
    kept_c = live_c if C_c is None else G.mask_C(live_c, C_c)
    idx = torch.from_numpy(kept_c)
    pts = q_c[idx].to(dtype)
    raw_c = forward(sd_c, pts) if pts.shape[0] else torch.zeros((0, 4), dtype=dtype)
    rgb_c, _, _, _, w_c = T.masked_outputs(raw_c, ts_c.to(dtype), dn.to(dtype), kept_c)
    ts_f = O.sample_pdf(ts_c.to(dtype), w_c.detach(), u_f.to(dtype))
    _, q_f, _ = T.geometry(rays.to(dtype), ts=ts_f)
    live_f = T.live_of(q_f.float(), cells, R, bounds, outside)
    kept_f = live_f if C_f is None else G.mask_C(live_f, C_f)
    loss_f = T.masked_loss(forward, sd_f, q_f, ts_f, dn, kept_f, gt, dtype)
    return torch.nn.functional.mse_loss(rgb_c, gt.to(dtype)), loss_f, live_c, live_f, ts_f
