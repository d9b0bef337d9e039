"""numpy restatement of the marching cubes of csrc/marching_cubes.hip (semantics: include/nerf_amd.h).

Same tables (tools/make_mc_tables.py), same order, same separately rounded float32 formulas: the GPU's vertices and
faces must equal this bit for bit, its normals to within 1e-6.  Also the mesh checks the tests apply to both.
"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_mc_tables", os.path.join(ROOT, "tools", "make_mc_tables.py"))
tables = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tables)

f32 = np.float32


def grid_step(lo, hi, R):
    """per-axis step fl32((hi - lo) / (R - 1)), computed in float32"""
    return [f32(f32(f32(h) - f32(l)) / f32(r - 1)) for l, h, r in zip(lo, hi, R)]


def grid_coords(lo, step, n):
    """x(i) = fl(lo + fl(i * s)) in float32"""
    i = np.arange(n, dtype=np.float32)
    return (f32(lo) + i * f32(step)).astype(np.float32)


def _gradient(sigma, coords):
    """d sigma / d axis at every grid point: central differences, one-sided on the grid's faces (float32)"""
    g = []
    for a in range(3):
        n = sigma.shape[a]
        hi = np.minimum(np.arange(n) + 1, n - 1)
        lo = np.maximum(np.arange(n) - 1, 0)
        x = coords[a]
        num = np.take(sigma, hi, axis=a) - np.take(sigma, lo, axis=a)
        den = (x[hi] - x[lo]).astype(np.float32)
        shape = [1, 1, 1]
        shape[a] = n
        g.append((num / den.reshape(shape)).astype(np.float32))
    return g


def marching_cubes(sigma, level, lo, step):
    """sigma [Rx,Ry,Rz] float32 (C order, z fastest) -> (verts [V,3] f32, faces [F,3] int32, normals [V,3] f32)"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):       # non-finite corners are part of the semantics
        return _marching_cubes(sigma, level, lo, step)


def _marching_cubes(sigma, level, lo, step):
    sigma = np.ascontiguousarray(sigma, dtype=np.float32)
    level = f32(level)
    R = sigma.shape
    coords = [grid_coords(lo[a], step[a], R[a]) for a in range(3)]
    finite = np.isfinite(sigma)
    inside = sigma > level
    grad = _gradient(sigma, coords)
    lin = np.arange(sigma.size, dtype=np.int64).reshape(R)

    # ---- vertices: one per crossing edge, ordered by (linear index of the lower endpoint, axis)
    keys, parts = [], []
    for a in range(3):
        sl_lo = [slice(None)] * 3
        sl_hi = [slice(None)] * 3
        sl_lo[a] = slice(0, R[a] - 1)
        sl_hi[a] = slice(1, R[a])
        sl_lo, sl_hi = tuple(sl_lo), tuple(sl_hi)
        cross = finite[sl_lo] & finite[sl_hi] & (inside[sl_lo] != inside[sl_hi])
        idx = np.nonzero(cross)
        la = lin[sl_lo][idx]
        sa, sb = sigma[sl_lo][idx], sigma[sl_hi][idx]
        t = ((level - sa) / (sb - sa)).astype(np.float32)
        ia = idx[a]
        xa, xb = coords[a][ia], coords[a][ia + 1]
        pos = np.empty((la.size, 3), np.float32)
        for b in range(3):
            pos[:, b] = coords[b][idx[b]]
        pos[:, a] = xa + t * (xb - xa)
        # normal: -grad interpolated with t between the endpoints, normalised; (0, 0, 0) for a zero or non-finite one
        ib = list(idx)
        ib[a] = ib[a] + 1
        ib = tuple(ib)
        one_t = (f32(1) - t).astype(np.float32)
        n = np.empty((la.size, 3), np.float32)
        for b in range(3):
            n[:, b] = -(one_t * grad[b][idx] + t * grad[b][ib])
        ln = np.sqrt((n.astype(np.float64) ** 2).sum(1))
        ok = np.isfinite(ln) & (ln > 0)
        nn = np.zeros_like(n)
        nn[ok] = (n[ok] / ln[ok, None]).astype(np.float32)
        keys.append(la * 3 + a)
        parts.append((pos, nn))
    key = np.concatenate(keys)
    order = np.argsort(key, kind="stable")
    verts = np.concatenate([p for p, _ in parts])[order]
    normals = np.concatenate([n for _, n in parts])[order]
    vid = np.full(sigma.size * 3, -1, np.int64)
    vid[key[order]] = np.arange(key.size)

    # ---- faces: cells in linear order, each case's triangles in table order; a cell with a non-finite corner emits none
    C = tuple(r - 1 for r in R)
    case = np.zeros(C, np.int64)
    allfin = np.ones(C, bool)
    for c in range(8):
        dx, dy, dz = tables.corner_offset(c)
        sl = (slice(dx, dx + C[0]), slice(dy, dy + C[1]), slice(dz, dz + C[2]))
        case |= inside[sl].astype(np.int64) << c
        allfin &= finite[sl]
    counts, tris = tables.build_tables()
    tri_count = np.array(counts, np.int64)
    mx = max(counts)
    tri_edges = np.full((256, mx, 3), -1, np.int64)
    for c in range(256):
        for k, t in enumerate(tris[c]):
            tri_edges[c, k] = t
    cells = np.nonzero(allfin & (tri_count[case] > 0))           # C order = linear cell order
    cc = case[cells]
    ntri = tri_count[cc]
    rep = np.repeat(np.arange(cc.size), ntri)
    k = np.arange(rep.size) - np.repeat(np.cumsum(ntri) - ntri, ntri)
    e = tri_edges[cc[rep], k]                                    # [F, 3] edge numbers
    lower = np.array([tables.edge_corners(j)[0] for j in range(12)])
    off = np.array([tables.corner_offset(c) for c in range(8)])
    base = np.stack([cells[b][rep] for b in range(3)], 1)       # [F, 3] cell origin
    faces = np.empty(e.shape, np.int64)
    for j in range(3):
        p = base + off[lower[e[:, j]]]
        li = (p[:, 0] * R[1] + p[:, 1]) * R[2] + p[:, 2]
        faces[:, j] = vid[li * 3 + e[:, j] // 4]
    assert (faces >= 0).all()
    return verts, faces.astype(np.int32), normals


# ---- mesh checks --------------------------------------------------------------------------------------------------
def directed_edges_closed(faces):
    """every directed edge exactly once and its reverse exactly once: closed, consistently oriented, 2 faces per edge"""
    f = faces.astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1 if f.size else 1
    key = d[:, 0] * n + d[:, 1]
    rkey = d[:, 1] * n + d[:, 0]
    uniq = np.unique(key)
    return uniq.size == key.size and np.array_equal(np.sort(key), np.sort(rkey))


def euler_characteristic(verts, faces):
    f = faces.astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = np.unique(np.sort(d, 1), axis=0)
    used = np.unique(f)
    return used.size - und.shape[0] + f.shape[0]


def area_and_volume(verts, faces):
    v = verts.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    cr = np.cross(b - a, c - a)
    area = 0.5 * np.linalg.norm(cr, axis=1).sum()
    vol = (a * np.cross(b, c)).sum() / 6.0
    return area, vol


# ---- analytic fields (raw-sigma-like: inside where positive) ---------------------------------------------------------
def grid_points(lo, hi, R):
    step = grid_step(lo, hi, R)
    xs = [grid_coords(lo[a], step[a], R[a]) for a in range(3)]
    X, Y, Z = np.meshgrid(*xs, indexing="ij")
    return X, Y, Z, step


def sphere_field(R, r=0.6, lo=(-1.0,) * 3, hi=(1.0,) * 3):
    X, Y, Z, step = grid_points(lo, hi, R)
    s = (f32(r * r) - (X * X + Y * Y + Z * Z)).astype(np.float32)
    return s, step


def torus_field(R, a=0.55, b=0.22, lo=(-1.0,) * 3, hi=(1.0,) * 3):
    X, Y, Z, step = grid_points(lo, hi, R)
    X, Y, Z = (v.astype(np.float64) for v in (X, Y, Z))
    q = np.sqrt(X * X + Y * Y) - a
    return (b * b - (q * q + Z * Z)).astype(np.float32), step


def gaussians_field(R, seed=0, n=6, lo=(-1.0,) * 3, hi=(1.0,) * 3):
    X, Y, Z, step = grid_points(lo, hi, R)
    rng = np.random.default_rng(seed)
    s = np.zeros(X.shape)
    for _ in range(n):
        c = rng.uniform(-0.6, 0.6, 3)
        w = rng.uniform(0.15, 0.35)
        s += rng.uniform(0.5, 1.5) * np.exp(-((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) / (2 * w * w))
    return (s - 0.5).astype(np.float32), step
