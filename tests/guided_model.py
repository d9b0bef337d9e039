"""numpy restatement of grid-guided fine sampling (include/nerf_amd.h, "grid-guided fine sampling"; csrc/guided_sample.hip):
the look-up -- the occupancy grid's cell rule and the NaN-skipping maximum over a cell's 8 corners -- and the composition
through the oracle's compositor and sample_pdf.  Test infrastructure: the look-up predicts every bit."""
import numpy as np
import torch

F32 = np.float32


def grid_axes(R, bounds):
    """(lo[3], step[3], inv_step[3]) in float32: step = fl((hi - lo) / (R - 1)), inv_step = fl(1 / step)."""
    lo = np.asarray(bounds[0], dtype=F32).reshape(3)
    hi = np.asarray(bounds[1], dtype=F32).reshape(3)
    step = ((hi - lo) / np.asarray([r - 1 for r in R], dtype=F32)).astype(F32)
    return lo, step, (F32(1) / step).astype(F32)


def points(rays, ts):
    """o + d t as every render forms it: float32, the product and the sum rounded separately -> [B, N, 3]."""
    rays, ts = np.asarray(rays, dtype=F32), np.asarray(ts, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (rays[:, None, :3] + (rays[:, None, 3:] * ts[:, :, None]).astype(F32)).astype(F32)


def cells(pts, R, lo, inv_step):
    """pts [..., 3] float32 -> (inside bool [...], index int64 [..., 3]): c = floor(fl(fl(x - lo) * inv_step)) per axis;
    outside when !(0 <= c < n - 1) on any axis (a NaN coordinate is outside).  The index of an outside point is 0."""
    p = np.asarray(pts, dtype=F32)
    inside = np.ones(p.shape[:-1], dtype=bool)
    idx = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            f = np.floor(((p[..., a] - lo[a]).astype(F32) * inv_step[a]).astype(F32))
            ok = (f >= F32(0)) & (f < F32(R[a] - 1))
            inside &= ok
            idx.append(np.where(ok, f, F32(0)).astype(np.int64))
    return inside, np.stack(idx, axis=-1)


def lookup(pts, V, lo, inv_step):
    """The value of each point: the maximum over the 8 corners of its cell, started from -inf, NaN corners skipped (a
    comparison with NaN is false); -inf outside the grid and in a cell whose corners are all NaN.  No arithmetic: exact."""
    V = np.asarray(V, dtype=F32)
    inside, c = cells(pts, V.shape, lo, inv_step)
    m = np.full(inside.shape, -np.inf, dtype=F32)
    with np.errstate(invalid="ignore"):
        for k in range(8):
            v = V[c[..., 0] + (k >> 2), c[..., 1] + ((k >> 1) & 1), c[..., 2] + (k & 1)]
            m = np.where(v > m, v, m)
    return np.where(inside, m, F32(-np.inf)).astype(F32)


def weights(oracle, rays, ts_c, value):
    """w [B, Nc] of the oracle's volume_render on raw = (0, 0, 0, value) with the rays' unit directions."""
    rays, ts_c = torch.as_tensor(rays, dtype=torch.float32), torch.as_tensor(ts_c, dtype=torch.float32)
    raw = torch.zeros(ts_c.shape + (4,), dtype=torch.float32)
    raw[..., 3] = torch.as_tensor(value, dtype=torch.float32)
    d = rays[:, 3:]
    return oracle.volume_render(raw, ts_c, d / torch.norm(d, dim=1, keepdim=True))[4]


def pdf(w):
    """The sampler's pdf over the Nc - 2 interior bins: (w[1:-1] + 1e-5) / sum."""
    wt = torch.as_tensor(w, dtype=torch.float32)[:, 1:-1] + 1e-5
    return wt / wt.sum(-1, keepdim=True)


def guided_sample(oracle, rays, ts_c, V, lo, inv_step, u_f):
    """The composition: points -> look-up -> oracle compositor -> oracle.sample_pdf -> (ts_out, sigma_c, w_c)."""
    sigma_c = lookup(points(rays, ts_c), V, lo, inv_step)
    w_c = weights(oracle, rays, ts_c, sigma_c)
    ts_out = oracle.sample_pdf(torch.as_tensor(ts_c, dtype=torch.float32), w_c, torch.as_tensor(u_f, dtype=torch.float32))
    return ts_out, sigma_c, w_c
