"""Geometry out of a trained ``Nerf``: density grids, marching cubes, PLY export.  Not in the reference.

    net = Nerf().cuda(); load_checkpoint(net, "model.pth")
    verts, faces, normals, rgb = extract_mesh(net, 256, colors=True)
    save_ply("model.ply", verts, faces, normals, torch.sigmoid(rgb))

* ``density_grid`` evaluates raw sigma (pre-softplus, column 3 of ``Nerf.forward``) on a regular grid.  For the default
  network in fp16 / bf16 the grid points are formed inside the sigma-only kernel (csrc/density.hip: layers 0..7 and the
  sigma row of layers_2, no input buffer), bit for bit ``net(points)[:, 3]``; fp32 and other network sizes run the
  existing forward on chunks of grid points that a small kernel writes (nerf_amd_grid_points).
* ``marching_cubes`` extracts the ``sigma > level`` surface of any fp32 device volume (csrc/marching_cubes.hip; the
  semantics are in include/nerf_amd.h): deterministic, closed and outward-oriented where the surface stays inside the grid.
* ``save_ply`` writes binary little-endian PLY on the host.

Grid coordinates, per axis: ``step = fl32((hi - lo) / (R - 1))`` and ``x(i) = fl32(lo + fl32(i * step))`` -- the same
numbers as torch's float32 ``lo + torch.arange(R) * step``.
"""
import warnings

import numpy as np
import torch

from .. import _lib
from .xyz import RANGE_WARNING

DEFAULT_BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
DEFAULT_LEVEL = 10.0
_CHUNK = 1 << 22                       # grid points per chunk of the fp32 / other-size fallback


def _resolution(resolution):
    r = (resolution,) * 3 if np.ndim(resolution) == 0 else tuple(resolution)
    if len(r) != 3 or any(int(x) != x or x < 2 or x > (1 << 24) for x in r):
        raise ValueError(f"resolution must be an integer or three integers in [2, 2^24], got {resolution!r}")
    return tuple(int(x) for x in r)


def grid_axes(resolution, bounds=DEFAULT_BOUNDS):
    """(lo[3], step[3]) as float32 numpy arrays: step = fl32((hi - lo) / (R - 1)), computed in float32."""
    R = _resolution(resolution)
    lo = np.asarray(bounds[0], dtype=np.float32).reshape(3)
    hi = np.asarray(bounds[1], dtype=np.float32).reshape(3)
    step = ((hi - lo) / np.asarray([r - 1 for r in R], dtype=np.float32)).astype(np.float32)
    return lo, step


def _warn_if_out_of_range(R, lo, step, stacklevel=3):
    """The reference's range warning (utils/xyz.py:8-9), decided on the host: Nerf.forward on the grid points (direction
    (0, 0, 1)) raises it iff a coordinate lies outside [-1, 1], and x(i) is monotone in i, so the two ends tell."""
    ends = np.stack([lo, (lo + (np.asarray(R, np.float32) - np.float32(1)) * step).astype(np.float32)])
    if np.any(ends < -1) or np.any(ends > 1):
        warnings.warn(RANGE_WARNING, UserWarning, stacklevel=stacklevel)


def density_grid(net, resolution, bounds=DEFAULT_BOUNDS, *, precision=None):
    """Raw sigma of ``net`` on an [Rx, Ry, Rz] grid over ``bounds = (lo[3], hi[3])`` (C order, z fastest) -> a float32
    device tensor; ``sigma[i, j, k]`` is ``net(points)[:, 3]`` at (x(i), y(j), z(k)) with any view direction.

    precision: as ``Nerf.forward`` (default: the module's).  fp16 / bf16 run under the range guard of the 16-bit kernels
    (utils/nets.guarded_launch): a non-finite value inside the network demotes fp16 to bf16 and bf16 to fp32, with a
    warning, and the grid is evaluated again."""
    R = _resolution(resolution)
    lo, step = grid_axes(R, bounds)
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("Nerf must be moved to the GPU (.cuda()) before use; there is no CPU path")
    _warn_if_out_of_range(R, lo, step)
    h_lo, h_step = _lib.host_f32x3(lo), _lib.host_f32x3(step)
    n = R[0] * R[1] * R[2]

    def by_chunks(forward):
        sigma = torch.empty(R, dtype=torch.float32, device=dev)
        flat = sigma.view(-1)
        pts = torch.empty((min(n, _CHUNK), 6), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):         # stays: the chunks' forward and the slice copy run under it too
            for first in range(0, n, _CHUNK):
                cnt = min(_CHUNK, n - first)
                _lib.launch("nerf_amd_grid_points", h_lo, h_step, R[0], R[1], R[2], first, cnt, pts, dev=dev)
                flat[first:first + cnt] = forward(pts[:cnt])[:, 3]
        return sigma

    with torch.no_grad():
        if not net._fused_ok():
            from . import generic_mlp
            return by_chunks(lambda p: generic_mlp.forward(net, p))
        from .nets import guarded_launch

        def launch(code, packed):
            if code == _lib.F32:
                return by_chunks(lambda p: net.forward_inference(p, precision="fp32"))
            sigma = torch.empty(R, dtype=torch.float32, device=dev)
            _lib.launch("nerf_amd_density_grid", h_lo, h_step, R[0], R[1], R[2], packed[0], code, sigma, dev=dev)
            return sigma

        code = _lib.precision_of(net, precision)
        return guarded_launch([net], code, launch)


def marching_cubes(volume, level, bounds=DEFAULT_BOUNDS):
    """Surface ``volume > level`` of a float32 device volume [Rx, Ry, Rz] (C order, z fastest) spanning ``bounds`` ->
    (verts [V,3] float32, faces [F,3] int32, normals [V,3] float32), all on the volume's device.  Semantics (vertex and face
    order, the interpolation, outward normals from central differences, non-finite corners): include/nerf_amd.h.
    One host synchronisation, for the counts."""
    _lib.require_cuda_f32(volume, "volume")
    if volume.dim() != 3:
        raise RuntimeError("marching_cubes expects a 3-D volume [Rx, Ry, Rz]")
    R = _resolution(tuple(volume.shape))
    lo, step = grid_axes(R, bounds)
    volume = volume.contiguous()
    dev = volume.device
    lib = _lib.lib()
    nbytes = int(lib.nerf_amd_marching_cubes_workspace_bytes(*R))
    if nbytes < 0:
        raise RuntimeError(f"marching_cubes: unsupported volume shape {R}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    lvl = float(level)
    _lib.launch("nerf_amd_marching_cubes_count", volume, *R, lvl, ws, counts, dev=dev)
    nv, nf = (int(x) for x in counts.cpu())
    if nv >= 1 << 31:
        raise RuntimeError(f"marching_cubes: {nv} vertices do not fit int32 face indices")
    verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    _lib.launch("nerf_amd_marching_cubes_emit", volume, *R, lvl, _lib.host_f32x3(lo), _lib.host_f32x3(step), ws, verts,
                normals, faces, nv, nf, dev=dev)
    return verts, faces, normals


def extract_mesh(net, resolution=256, level=DEFAULT_LEVEL, bounds=DEFAULT_BOUNDS, *, colors=False, precision=None):
    """The ``sigma > level`` surface of ``net`` over ``bounds`` on a resolution^3 (or [Rx, Ry, Rz]) grid:
    ``marching_cubes(density_grid(net, resolution, bounds), level, bounds)`` -> (verts [V,3], faces [F,3] int32,
    normals [V,3]), plus, with ``colors=True``, rgb [V,3] = ``net(cat[verts, -normals])[:, :3]``: the raw colour (apply
    torch.sigmoid as the compositor does) seen looking at the surface along its inward normal.

    level is in raw-sigma units, the network's column 3.  The compositor uses softplus(sigma) as the volume density
    (utils/rendering.py); softplus(sigma) = sigma + log(1 + exp(-sigma)) is sigma to within 2e-9 above 20 and within
    5e-5 at the default 10, so a level above ~10 is also the density level."""
    vol = density_grid(net, resolution, bounds, precision=precision)
    verts, faces, normals = marching_cubes(vol, level, bounds)
    if not colors:
        return verts, faces, normals
    with torch.no_grad():
        if verts.shape[0] == 0:
            rgb = torch.empty((0, 3), dtype=torch.float32, device=verts.device)
        else:
            rgb = net(torch.cat([verts, -normals], 1), precision=precision)[:, :3]
    return verts, faces, normals, rgb


def save_ply(path, verts, faces, normals=None, colors=None):
    """Binary little-endian PLY: vertices (x, y, z float32, [nx, ny, nz float32], [red, green, blue uchar]) and faces
    (uchar count, int32 indices).  colors: uint8, or floats in [0, 1] (rounded, clipped).  Tensors or arrays."""
    def host(a, dtype):
        if a is None:
            return None
        if torch.is_tensor(a):
            a = a.detach().cpu().numpy()
        return np.ascontiguousarray(a, dtype=dtype) if dtype is not None else np.asarray(a)

    v = host(verts, np.float32).reshape(-1, 3)
    f = host(faces, np.int32).reshape(-1, 3)
    n = host(normals, np.float32)
    c = host(colors, None)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if n is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if c is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        if c.dtype != np.uint8:
            c = np.rint(np.clip(c.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
        c = c.reshape(-1, 3)
    vrec = np.empty(v.shape[0], dtype=fields)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if n is not None:
        n = n.reshape(-1, 3)
        vrec["nx"], vrec["ny"], vrec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if c is not None:
        vrec["red"], vrec["green"], vrec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"] = 3
    frec["v"] = f
    names = {"<f4": "float", "u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    header += [f"property {names[t]} {k}" for k, t in fields]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())
    return path
