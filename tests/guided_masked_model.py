"""numpy restatement of the masked guided placement (include/nerf_amd.h, "masked guided placement"; csrc/guided_masked.hip;
DESIGN.md section 24): the six steps of the definition, composed from guided_model (points, look-up, weights) and
occupancy_model (the cell of a point and its bit, mask words, offsets) and the oracle's sample_pdf -- nothing of them is
restated here.  Test infrastructure: the look-ups predict every bit."""
import numpy as np
import torch

import guided_model as G
import occupancy_model as OM

F32 = np.float32


def masked_guided_sample(oracle, rays, ts_c, V, v_lo, v_inv_step, cells, g_lo, g_inv_step, outside, u_f):
    """-> dict: ts [B, Nc+Nf], sigma_c (AFTER the coarse masking), w_c, live_c bool [B, Nc], live bool [B, Nc+Nf],
    mask uint64 [B, ceil((Nc+Nf)/64)], offsets int64 [B+1]."""
    ts_c = torch.as_tensor(ts_c, dtype=torch.float32)
    pts = G.points(rays, ts_c)                                                        # 1. the coarse points
    value = G.lookup(pts, V, v_lo, v_inv_step)                                        # 2. the look-up in V
    live_c = OM.sample_live(pts, cells, g_lo, g_inv_step, outside)                    # 3. the grid at the coarse samples
    sigma_c = np.where(live_c, value, F32(-np.inf)).astype(F32)
    w_c = G.weights(oracle, rays, ts_c, sigma_c)                                      # 4. the compositor's weights
    ts = oracle.sample_pdf(ts_c, w_c, torch.as_tensor(u_f, dtype=torch.float32))      # 5. the sampler
    live = OM.sample_live(G.points(rays, ts), cells, g_lo, g_inv_step, outside)       # 6. the grid at the merged positions
    return {"ts": ts, "sigma_c": sigma_c, "w_c": w_c, "live_c": live_c, "live": live, "mask": OM.mask_words(live),
            "offsets": OM.offsets(live)}


def live_bin_mass(w_c, live_c):
    """The sampler's pdf mass in the bins of the live coarse samples (interior bins 1 .. Nc-2) -> [B]."""
    return (G.pdf(w_c) * torch.from_numpy(np.asarray(live_c))[:, 1:-1]).sum(1)


def slab_rays():
    """The 36-ray slab set of test_guided_cpu.test_model_hot_slab_takes_the_pdf_mass: from z = 4 down through the box, aimed
    at a 6 x 6 lattice on the plane z = 0, unit directions."""
    aim = torch.stack(torch.meshgrid(torch.linspace(-1, 1, 6), torch.linspace(-1, 1, 6), indexing="ij"), -1).reshape(-1, 2)
    o = torch.tensor([0.3, -0.2, 4.0]).expand(aim.shape[0], 3)
    d = torch.cat([aim, torch.zeros(aim.shape[0], 1)], 1) - o
    return torch.cat([o, d / torch.norm(d, dim=1, keepdim=True)], 1).contiguous()


def slab_cells(R=(33, 33, 33)):
    """Cells 13 .. 18 along z live, every other cell dead."""
    c = np.zeros(tuple(r - 1 for r in R), dtype=bool)
    c[:, :, 13:19] = True
    return c


def stratified(B, Nc, seed, tn=2, tf=6):
    """ts_c [B, Nc] of torch.rand(B, Nc) under this generator seed, as render_nerf forms them."""
    u = torch.rand(B, Nc, generator=torch.Generator().manual_seed(seed))
    tb = torch.linspace(tn, tf, Nc + 1)
    return (tb[1] - tb[0]) * u + tb[:-1]
