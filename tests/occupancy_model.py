"""numpy restatement of the occupancy grid and the masked render (include/nerf_amd.h; csrc/occupancy.hip): the bit
packing, the corner / dilation rule, the cell of a point, the per-ray masks and offsets, and the masked composition through
the oracle's volume_render with (0, 0, 0, -inf) rows.  Test infrastructure: predicts every bit of every mask."""
import numpy as np
import torch

F32 = np.float32


def grid_axes(R, bounds):
    """(lo[3], step[3], inv_step[3]) in float32: step = fl((hi - lo) / (R - 1)), inv_step = fl(1 / step)."""
    lo = np.asarray(bounds[0], dtype=F32).reshape(3)
    hi = np.asarray(bounds[1], dtype=F32).reshape(3)
    step = ((hi - lo) / np.asarray([r - 1 for r in R], dtype=F32)).astype(F32)
    return lo, step, (F32(1) / step).astype(F32)


def words_per_row(R):
    return (R[2] - 1 + 31) // 32


def grid_words(R):
    return (R[0] - 1) * (R[1] - 1) * words_per_row(R)


def pack_bits(cells):
    """bool [Cx, Cy, Cz] -> uint32 [Cx * Cy * Wz]: z fastest, 32 cells per word, rows padded with zero bits."""
    cells = np.asarray(cells, dtype=bool)
    cx, cy, cz = cells.shape
    wz = (cz + 31) // 32
    padded = np.zeros((cx, cy, wz * 32), dtype=np.uint64)
    padded[:, :, :cz] = cells
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (padded.reshape(cx, cy, wz, 32) * weights).sum(-1).astype(np.uint32).reshape(-1)


def unpack_bits(words, R):
    cx, cy, cz = (r - 1 for r in R)
    wz = (cz + 31) // 32
    w = np.asarray(words).view(np.uint32).reshape(cx, cy, wz, 1)
    bits = (w >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(cx, cy, wz * 32)[:, :, :cz].astype(bool)


def cells_from_density(sigma, level, dilate):
    """A cell is dead iff every corner of every cell within `dilate` cells of it (Chebyshev, clipped) has sigma <= level."""
    with np.errstate(invalid="ignore"):
        hot = ~(np.asarray(sigma, dtype=F32) <= F32(level))           # NaN is hot
    c = np.zeros(tuple(n - 1 for n in hot.shape), dtype=bool)
    for a in (0, 1):
        for b in (0, 1):
            for d in (0, 1):
                c |= hot[a:a + c.shape[0], b:b + c.shape[1], d:d + c.shape[2]]
    for axis in range(3):                                           # a box maximum is separable
        out = c.copy()
        for s in range(1, dilate + 1):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, c.shape[axis] - s), slice(s, None)
            if c.shape[axis] > s:
                out[tuple(lo)] |= c[tuple(hi)]
                out[tuple(hi)] |= c[tuple(lo)]
        c = out
    return c


def cells_from_density_direct(sigma, level, dilate):
    """The same rule spelt out cell by cell (slow; small volumes only): the check of the separable form above."""
    with np.errstate(invalid="ignore"):
        hot = ~(np.asarray(sigma, dtype=F32) <= F32(level))
    C = tuple(n - 1 for n in hot.shape)
    out = np.zeros(C, dtype=bool)
    for i in range(C[0]):
        for j in range(C[1]):
            for k in range(C[2]):
                sl = tuple(slice(max(v - dilate, 0), min(v + dilate, n - 1) + 2) for v, n in zip((i, j, k), C))
                out[i, j, k] = hot[sl].any()
    return out


def ball_cells(R, bounds, radius):
    """cell mask of a ball around the origin, judged at the cell centre"""
    lo = np.asarray(bounds[0], dtype=np.float64)
    hi = np.asarray(bounds[1], dtype=np.float64)
    axes = [lo[a] + (np.arange(R[a] - 1) + 0.5) * (hi[a] - lo[a]) / (R[a] - 1) for a in range(3)]
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    return X * X + Y * Y + Z * Z <= radius * radius


def sample_live(points, cells, lo, inv_step, outside):
    """points [..., 3] float32 -> bool [...]: c = floor(fl(fl(x - lo) * inv_step)) per axis in float32; c < 0, c >= C or NaN
    on any axis is outside (live iff outside == 'live'), otherwise the cell's bit."""
    p = np.asarray(points, dtype=F32)
    C = cells.shape
    inside = np.ones(p.shape[:-1], dtype=bool)
    idx = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            f = np.floor(((p[..., a] - lo[a]).astype(F32) * inv_step[a]).astype(F32))
            ok = (f >= F32(0)) & (f < F32(C[a]))
            inside &= ok
            idx.append(np.where(ok, f, F32(0)).astype(np.int64))
    return np.where(inside, cells[idx[0], idx[1], idx[2]], outside == "live")


def mask_words(live):
    """bool [B, N] -> uint64 [B, ceil(N / 64)]"""
    B, N = live.shape
    W = (N + 63) // 64
    padded = np.zeros((B, W * 64), dtype=np.uint64)
    padded[:, :N] = live
    return (padded.reshape(B, W, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def offsets(live):
    out = np.zeros(live.shape[0] + 1, dtype=np.int64)
    np.cumsum(live.sum(1), out=out[1:])
    return out


def stats(live):
    """(live fraction, most live samples on one ray, share of rays with no live sample)"""
    per_ray = live.sum(1)
    return float(live.mean()), int(per_ray.max()), float((per_ray == 0).mean())


def require_informative(live, N, outside):
    """The inputs of a masking test must not degenerate to all or nothing (fails loudly, never skips)."""
    frac, fullest, empty = stats(live)
    assert 0.02 < frac < 0.6, f"live fraction {frac} outside (0.02, 0.6)"
    assert fullest >= -(-N // 4), f"fullest ray has {fullest} live samples, fewer than ceil(N / 4)"
    if outside == "empty":
        assert empty > 0, "no ray without a live sample under outside='empty'"
    return frac, fullest, empty


def masked_raw(raw, live):
    """raw [B, N, 4] with (0, 0, 0, -inf) at the dead samples"""
    raw = raw.clone()
    dead = torch.from_numpy(~np.asarray(live))
    raw[dead] = torch.tensor([0.0, 0.0, 0.0, -np.inf], dtype=raw.dtype)
    return raw


def masked_composite(oracle, raw, ts, dirs, live):
    """The masked render's definition: the oracle's volume_render over all N samples with the dead rows replaced."""
    return oracle.volume_render(masked_raw(raw, live), ts, dirs)


def live_only_composite(raw, ts, dirs, live):
    """A composite that never looks at a dead sample: the weights of the live samples from the oracle's formulas (delta =
    distance to the NEXT SAMPLE POSITION, dead or not; transmittance = running product of the live samples' factors before it),
    accumulated ray by ray over the live samples alone in sample order.  Returns (rgb, depth, acc, alpha, w), alpha / w
    [B, N] with zeros at the dead samples."""
    live = torch.from_numpy(np.asarray(live))
    B, N = ts.shape
    deltas = torch.cat((ts[:, 1:] - ts[:, :-1], 1e10 * torch.ones_like(ts[:, :1])), dim=1)
    deltas = deltas * torch.norm(dirs[..., None, :], dim=-1)
    alpha = torch.zeros_like(ts)
    w = torch.zeros_like(ts)
    T = torch.ones(B, dtype=torch.float64)      # torch.cumprod on the CPU accumulates float32 factors in double
    rgb = torch.zeros(B, 3, dtype=ts.dtype)
    depth = torch.zeros(B, dtype=ts.dtype)
    acc = torch.zeros(B, dtype=ts.dtype)
    for i in range(N):
        m = live[:, i]
        a = 1 - torch.exp(-torch.nn.functional.softplus(raw[:, i, 3]) * deltas[:, i])
        wi = a * T.to(ts.dtype)
        alpha[:, i] = torch.where(m, a, alpha[:, i])
        w[:, i] = torch.where(m, wi, w[:, i])
        rgb = torch.where(m[:, None], rgb + wi[:, None] * raw[:, i, :3], rgb)
        depth = torch.where(m, depth + wi * ts[:, i], depth)
        acc = torch.where(m, acc + wi, acc)
        # a dead sample's factor is 1 - 0 + 1e-10 as the dtype rounds it: exactly 1 in float32 (float64 keeps the 1e-10)
        T = T * torch.where(m, 1. - a + 1e-10, 1. - torch.zeros_like(a) + 1e-10).double()
    return rgb, depth, acc, alpha, w


def sequential_sums(w, raw, ts):
    """sum_i w_i c_i, sum_i w_i t_i, sum_i w_i accumulated in sample order over ALL samples (the order live_only_composite
    uses on the live ones)"""
    B, N = ts.shape
    rgb = torch.zeros(B, 3, dtype=ts.dtype)
    depth = torch.zeros(B, dtype=ts.dtype)
    acc = torch.zeros(B, dtype=ts.dtype)
    for i in range(N):
        rgb = rgb + w[:, i, None] * raw[:, i, :3]
        depth = depth + w[:, i] * ts[:, i]
        acc = acc + w[:, i]
    return rgb, depth, acc
