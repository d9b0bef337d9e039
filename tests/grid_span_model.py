"""The grid span's placement (include/nerf_amd.h "grid span", csrc/grid_span_device.h) restated on the CPU: op for op in fp32 --
what nerf_amd_span_positions must equal bit for bit -- and once more in float64.  The clip and the placement are
tests/box_model.py's ``span`` / ``place``, the grid is tests/occupancy_model.py's; only the K segments are new here.  Nothing
is taken from what a GPU shows.

Definition, per ray (o, d), grid of C = R - 1 cells per axis over [lo, hi] with inv_step = fl(1 / step), K segments (every
operation rounded on its own, no fma):
    [a, b], inside = box_model.span(ray, lo, hi, tn, tf)           a slab miss: hit = 0, [tn, tf], nothing is read
    e_0 = a, e_K = b, e_j = fl(a + fl(fl(b - a) * fl(j / K)))      the K + 1 edges
    p_j = fl(o + fl(e_j * d)) per axis, c_j = clamp(floor(fl(fl(p_j - lo) * inv_step)), 0, C - 1)   (a NaN -> 0)
    segment j is live iff a bit is set among the 8 cells (c_j | c_j+1)_x x (c_j | c_j+1)_y x (c_j | c_j+1)_z
    j0 / j1 the first / last live segment: t0 = e_j0, t1 = e_(j1 + 1), hit = 1;   none: hit = 0, [tn, tf]
    ts_i = min(t0 + (t1 - t0) c_i, t1) on the unit positions c (box_model.unit_positions)

Why the 8 cells are enough, and what "conservative" means: with K >= 2 max(C) and [a, b] inside the grid's bounds, a segment
is at most (hi - lo) sqrt(3) / K long in space -- at most half a cell per axis -- so it touches at most two cells per axis,
the cells of its two end points, and every cell it crosses is among the 8.  A point of the ray in [a, b] that lies in a live
cell therefore lies in a live segment, and [t0, t1] contains every live segment.  fp32 enters at a cell face only: the mark
kernel floors its own fl(o + fl(t d)), the span floors the edges', and the two may fall on either side of a face for a t within
a rounding of it -- which is why the conservativeness test allows one segment length, and finds it does not need it.
"""
import numpy as np
import torch

import box_model as BM
import occupancy_model as OM

F32 = np.float32


class Grid:
    """A cell mask with the axes the package derives for it: ``cells`` bool [Cx, Cy, Cz], ``R``, ``bounds``, and lo / hi /
    inv_step as fp32 triples (hi is the bound itself, as the entry point takes it)."""

    def __init__(self, cells, bounds):
        self.cells = np.asarray(cells, dtype=bool)
        self.R = tuple(c + 1 for c in self.cells.shape)
        self.bounds = bounds
        self.lo, self.step, self.inv_step = OM.grid_axes(self.R, bounds)
        self.hi = np.asarray(bounds[1], dtype=F32).reshape(3)

    def least_probes(self):
        return max(64, -(-2 * max(self.cells.shape) // 64) * 64)


def edges(a, b, K):
    """e [B, K + 1] in the dtype of ``a``: the ends are a and b themselves."""
    dt = a.dtype.type
    frac = np.arange(K + 1).astype(dt) / dt(K)
    with np.errstate(invalid="ignore", over="ignore"):
        e = a[:, None] + (b - a)[:, None] * frac[None, :]
    e[:, 0], e[:, K] = a, b
    return e


def cell_index(p, lo, inv_step, C):
    """floor(fl(fl(p - lo) * inv_step)) clamped into [0, C - 1] by the kernel's two comparisons: NaN -> 0."""
    dt = p.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((p - dt(lo)) * dt(inv_step))
        f = np.where(f >= 1, np.where(f < C - 1, f, dt(C - 1)), dt(0))
    return f.astype(np.int64)


def segments_live(rays, e, grid):
    """bool [B, K]: segment j's 8 cells hold a live one.  ``rays`` numpy [B, 6] in the dtype of ``e``."""
    idx = []
    with np.errstate(invalid="ignore", over="ignore"):
        for x in range(3):
            p = rays[:, x, None] + e * rays[:, 3 + x, None]
            idx.append(cell_index(p, grid.lo[x], grid.inv_step[x], grid.cells.shape[x]))
    live = np.zeros((e.shape[0], e.shape[1] - 1), dtype=bool)
    for k in range(8):
        cx, cy, cz = (idx[x][:, 1:] if (k >> (2 - x)) & 1 else idx[x][:, :-1] for x in range(3))
        live |= grid.cells[cx, cy, cz]
    return live


def span(rays, grid, K, tn, tf):
    """(t0 [B], t1 [B], hit [B] bool, clip) as torch tensors in the dtype of ``rays`` (float32: the kernel's operations one by
    one; float64: the same formula); ``clip`` = (a, b, inside) of the slab step."""
    a, b, inside = BM.span(rays, [float(x) for x in grid.lo], [float(x) for x in grid.hi], tn, tf)
    r, an, bn = rays.numpy(), a.numpy(), b.numpy()
    e = edges(an, bn, K)
    live = segments_live(r, e, grid) & inside.numpy()[:, None]
    hit = live.any(axis=1)
    j0 = live.argmax(axis=1)
    j1 = K - 1 - live[:, ::-1].argmax(axis=1)
    rows = np.arange(r.shape[0])
    dt = an.dtype.type
    t0 = np.where(hit, e[rows, j0], dt(tn))
    t1 = np.where(hit, e[rows, j1 + 1], dt(tf))
    return torch.from_numpy(t0), torch.from_numpy(t1), torch.from_numpy(hit), (a, b, inside)


def positions(rays, grid, K, tn, tf, c):
    """(ts [B,N], span [B,2], hit [B] int32) for unit positions c [B,N], in the dtype of ``rays`` and ``c``."""
    t0, t1, hit, _ = span(rays, grid, K, tn, tf)
    return BM.place(t0, t1, c), torch.stack([t0, t1], dim=1), hit.to(torch.int32)


def live_positions(rays, ts, grid):
    """bool [B, N]: what the mark kernel says of these positions behind outside='empty' (occupancy_model.sample_live on
    fl(o + fl(t d)))."""
    r, t = rays.numpy().astype(F32), np.asarray(ts, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        pts = r[:, None, :3] + (t[:, :, None] * r[:, None, 3:]).astype(F32)
    return OM.sample_live(pts.astype(F32), grid.cells, grid.lo, grid.inv_step, "empty")


# ---- the grids of the tests ----------------------------------------------------------------------------------------------------
BALL_R, BALL_BOUNDS = (129, 129, 129), ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
HAND_R, HAND_BOUNDS = (9, 5, 7), ((-2.0, -1.0, -1.5), (2.0, 1.0, 1.5))
R33 = (33, 33, 33)


def ball():
    return Grid(OM.ball_cells(BALL_R, BALL_BOUNDS, 1.0), BALL_BOUNDS)


def hand_made():
    """8 x 4 x 6 cells of side 0.5: one interior cell, one corner cell on the grid's edge, and two cells with a gap between
    them on the ray along +x through y = -0.75, z = 0.25 (``gap_ray``)."""
    cells = np.zeros((8, 4, 6), dtype=bool)
    cells[3, 2, 2] = True
    cells[7, 3, 0] = True
    cells[1, 0, 3] = cells[5, 0, 3] = True
    return Grid(cells, HAND_BOUNDS)


def gap_ray():
    """From x = -5 along +x through the two cells of ``hand_made`` with the gap: cell 1 spans x in [-1.5, -1], cell 5 spans
    [0.5, 1], so t0 ~ 3.5 and t1 ~ 6 clip at tf = 6 exactly: [3.5, 6]."""
    return [-5.0, -0.75, 0.25, 1.0, 0.0, 0.0]


def ball33():
    return Grid(OM.ball_cells(R33, BALL_BOUNDS, 1.0), BALL_BOUNDS)


def all_live(R=(9, 5, 7), bounds=HAND_BOUNDS):
    return Grid(np.ones(tuple(r - 1 for r in R), dtype=bool), bounds)


def all_dead(R=(9, 5, 7), bounds=HAND_BOUNDS):
    return Grid(np.zeros(tuple(r - 1 for r in R), dtype=bool), bounds)
