"""The scene box: each ray's sampling interval clipped to an axis-aligned box.  Not in the reference, whose samples lie
in ``linspace(tn, tf, N + 1)`` bins whatever the ray (utils/rendering.py:24-30).  DESIGN.md section 33.

    box = SceneBox.from_occupancy(occ)                                    # the live cells' own box, once per grid update
    pixels = render_view(net, pose, cam_params, device_rng=True, occupancy=occ, box=box)
    loss = train_step(net, opt, rays, gt, 64, device_rng=True, seed=step, occupancy=occ, box=box)
    ts = box.positions(rays, 64, device_rng=True)                         # or place them yourself and pass ts=

Per ray the N samples are placed in [t0, t1] = [tn, tf] cut by the box's slabs, by the jitter rule every render uses, on
unit bins (nerf_amd_box_positions: include/nerf_amd.h states the definition, tests/box_model.py restates it op for op).  A
ray that misses the box keeps [tn, tf]: it renders as it does without a box, and behind a grid whose outside is empty it is
dead as a whole.  The positions are CONSTANTS of the render, as the fine sampler's are: they carry no gradient, and
``d loss / d rays`` ignores the dependence of t0 and t1 on the ray.  The distortion term keeps the global ``tf`` and its
coefficient lambda / (B (tf - tn)): the last sample still owns [t_last, tf].

``box=`` on an entry point resolves the box to ``ts`` once, before anything else is drawn, and then IS that entry point's
``ts=`` path; with ``box=None`` the call is the call it was.

The grid span is the box's successor: ``GridSpan(occ)`` cuts each ray's interval from the occupancy
grid's own bits on the device -- from the ray's first live cell to its last (nerf_amd_span_positions; tests/grid_span_model.py)
-- and is accepted wherever ``box=`` is.  It holds the grid, not a copy: ``occ.update()`` is seen by the next call.

    span = GridSpan(occ)                                                  # once; follows occ.update() by itself
    loss = train_step(net, opt, rays, gt, 24, device_rng=True, seed=step, occupancy=occ, box=span)
"""
import math

import numpy as np
import torch

from .. import _lib
from . import jitter

MAX_N = 768                             # samples per ray of the entry points that read the positions (the masked stages)


class SceneBox:
    """``SceneBox(lo, hi)``: an axis-aligned box as one frozen, validated value -- two triples of finite floats (held
    rounded to fp32, as the kernel sees them) with lo < hi on every axis; ValueError otherwise."""

    __slots__ = ("lo", "hi")

    def __init__(self, lo, hi):
        def triple(v, name):
            try:
                with np.errstate(over="ignore"):         # a value beyond fp32 becomes inf and is refused below
                    t = tuple(float(np.float32(x)) for x in v)
            except TypeError:
                raise ValueError(f"SceneBox: {name} must be three numbers, got {v!r}") from None
            if len(t) != 3 or not all(math.isfinite(x) for x in t):
                raise ValueError(f"SceneBox: {name} must be three finite numbers, got {v!r}")
            return t
        lo, hi = triple(lo, "lo"), triple(hi, "hi")
        if not all(a < b for a, b in zip(lo, hi)):
            raise ValueError(f"SceneBox: lo < hi on every axis, got lo = {lo}, hi = {hi}")
        object.__setattr__(self, "lo", lo)
        object.__setattr__(self, "hi", hi)

    def __setattr__(self, name, value=None):
        raise AttributeError(f"SceneBox is frozen: build a new one to change {name!r}")

    __delattr__ = __setattr__

    def __repr__(self):
        return f"SceneBox(lo={self.lo!r}, hi={self.hi!r})"

    def __eq__(self, other):
        return isinstance(other, SceneBox) and (self.lo, self.hi) == (other.lo, other.hi)

    def __hash__(self):
        return hash((self.lo, self.hi))

    # ---- construction ---------------------------------------------------------------------------------------------------
    @classmethod
    def from_grid(cls, g):
        """The bounds of an ``OccupancyGrid``, a ``TrainingOccupancyGrid`` or a ``ProposalVolume``."""
        bounds = getattr(g, "bounds", None)
        if bounds is None or len(bounds) != 2:
            raise TypeError("SceneBox.from_grid takes an OccupancyGrid, a TrainingOccupancyGrid or a ProposalVolume")
        return cls(bounds[0], bounds[1])

    @classmethod
    def from_occupancy(cls, occ, margin=1):
        """The box of the grid's LIVE cells, widened by ``margin`` cells and clamped to the grid's bounds: the tight box.
        Plain torch on the unpacked bits and one host read -- call it when the grid changes, not per step.  A grid with no
        live cell raises ValueError."""
        from .occupancy import OccupancyGrid
        if not isinstance(occ, OccupancyGrid):
            raise TypeError("SceneBox.from_occupancy takes an OccupancyGrid (utils/occupancy.py)")
        if int(margin) != margin or margin < 0:
            raise ValueError(f"margin must be a non-negative integer (cells), got {margin!r}")
        return cls(*_live_bounds(occ.cells(), occ.lo, occ.step, occ.bounds, int(margin)))

    # ---- placement ------------------------------------------------------------------------------------------------------
    def positions(self, rays, N, tn=2, tf=6, *, u=None, ts=None, device_rng=False, seed=0, ray_id0=0, return_span=False):
        """ts [B, N]: the sample positions of ``rays`` inside this box (nerf_amd_box_positions).  Jitter as ``render_nerf``:
        ``u`` [B, N] uniforms, ``device_rng`` the counter RNG keyed by (seed, ray_id0 + ray), default one reference
        ``torch.rand(B, N)`` continued on the device; ``ts`` [B, N] are UNIT positions of the caller's own (0 = t0, 1 = t1).
        ``return_span=True``: (ts, span [B, 2] = (t0, t1), hit [B] int32).  The positions carry no gradient, and nothing else does.  A refused call
        leaves torch's generator where it was."""
        return _positions(self, rays, N, tn, tf, u, ts, device_rng, seed, ray_id0, return_span)

    def placement(self, dev):
        """(entry point, its arguments between ``ray_id0`` and ``tn``): how ``place`` and the graphed steppers launch this box."""
        return "nerf_amd_box_positions", (_lib.host_f32x3(self.lo), _lib.host_f32x3(self.hi))


MAX_SPAN_CELLS, MAX_PROBES = 512, 1024  # cells per axis and segments nerf_amd_span_positions serves (probes >= 2 cells)


class GridSpan:
    """``GridSpan(occupancy, probes=None)``: each ray's interval from its first to its last live cell of ``occupancy`` (an
    ``OccupancyGrid`` / ``TrainingOccupancyGrid`` whose outside is empty), cut on the device from the grid's bits in place --
    a frozen, validated value that HOLDS the grid object, so an in-place ``update()`` is seen by the next placement.
    ``probes``: the segments K a ray's clipped interval is cut into, a multiple of 64 with 2 max(cells per axis) <= K <= 1024;
    None takes the smallest (256 for a 129^3 grid).  ValueError for an ``outside='live'`` grid (the span speaks for the cells
    only: what lies outside them would be live and unseen), a bad ``probes`` or a grid beyond 512 cells per axis."""

    __slots__ = ("occupancy", "probes")

    def __init__(self, occupancy, probes=None):
        from .occupancy import OccupancyGrid
        if not isinstance(occupancy, OccupancyGrid):
            raise TypeError("GridSpan takes an OccupancyGrid (utils/occupancy.py)")
        if occupancy.outside != "empty":
            raise ValueError("GridSpan needs a grid with outside='empty': behind outside='live' the samples outside the grid "
                             "are live, and the span of the grid's cells does not cover them")
        cells = max(r - 1 for r in occupancy.resolution)
        if cells > MAX_SPAN_CELLS:
            raise ValueError(f"GridSpan serves grids of up to {MAX_SPAN_CELLS} cells per axis, got {cells}")
        least = max(64, -(-2 * cells // 64) * 64)
        if probes is None:
            probes = least
        elif isinstance(probes, bool) or int(probes) != probes or probes % 64 or not least <= probes <= MAX_PROBES:
            raise ValueError(f"probes must be a multiple of 64 in [{least}, {MAX_PROBES}] for this grid (at least twice its "
                             f"{cells} cells per axis), got {probes!r}")
        object.__setattr__(self, "occupancy", occupancy)
        object.__setattr__(self, "probes", int(probes))

    def __setattr__(self, name, value=None):
        raise AttributeError(f"GridSpan is frozen: build a new one to change {name!r}")

    __delattr__ = __setattr__

    def __repr__(self):
        return f"GridSpan({type(self.occupancy).__name__}{tuple(self.occupancy.resolution)!r}, probes={self.probes})"

    def __eq__(self, other):
        return isinstance(other, GridSpan) and self.occupancy is other.occupancy and self.probes == other.probes

    def __hash__(self):
        return hash((id(self.occupancy), self.probes))

    def positions(self, rays, N, tn=2, tf=6, *, u=None, ts=None, device_rng=False, seed=0, ray_id0=0, return_span=False):
        """ts [B, N]: the sample positions of ``rays`` between each ray's first and last live cell (nerf_amd_span_positions),
        read from the grid's bits as they are now.  Arguments, jitter and returns as ``SceneBox.positions``: ``u`` [B, N]
        uniforms, ``device_rng`` the counter RNG keyed by (seed, ray_id0 + ray), default one reference ``torch.rand(B, N)``;
        ``ts`` [B, N] are UNIT positions of the caller's own.  ``return_span=True``: (ts, span [B, 2], hit [B] int32); a ray
        that meets no live cell has hit = 0 and keeps [tn, tf].  The positions carry no gradient, and nothing else does.  A
        refused call leaves torch's generator where it was."""
        return _positions(self, rays, N, tn, tf, u, ts, device_rng, seed, ray_id0, return_span)

    def placement(self, dev):
        occ = self.occupancy
        _lib.require_same_device("occupancy grid", occ.words, dev)
        return "nerf_amd_span_positions", (occ.words, *occ.resolution, _lib.host_f32x3(occ.lo), _lib.host_f32x3(occ.bounds[1]),
                                           _lib.host_f32x3(occ.inv_step), self.probes)


def _positions(box, rays, N, tn, tf, u, ts, device_rng, seed, ray_id0, return_span):
    """``SceneBox.positions`` / ``GridSpan.positions``: the checks, the jitter, one placement."""
    B, N = _lib.require_rays(rays), int(N)
    check_interval(N, tn, tf)
    if isinstance(box, GridSpan):
        _lib.require_same_device("occupancy grid", box.occupancy.words, rays.device)
    jit, flags, pending = jitter.single(B, N, rays.device, u=u, ts=ts, device_rng=device_rng)
    try:
        out = place(box, rays.detach().contiguous(), jit, flags, seed, ray_id0, N, tn, tf, return_span)
    finally:
        if pending is not None:
            pending.finish()
    return out if return_span else out[0]


def _live_bounds(cells, lo, step, bounds, margin):
    """(lo[3], hi[3]) of the live entries of the bool cell mask [Cx, Cy, Cz]: cell i of an axis spans
    [lo + i step, lo + (i + 1) step]; an end that reaches the grid's edge is the grid's own bound."""
    if not bool(cells.any()):
        raise ValueError("SceneBox.from_occupancy: the grid has no live cell")
    box_lo, box_hi = [], []
    for a in range(3):
        live = torch.nonzero(cells.any(dim=tuple(d for d in range(3) if d != a))).flatten()
        C = cells.shape[a]
        i0, i1 = max(int(live[0]) - margin, 0), min(int(live[-1]) + 1 + margin, C)
        box_lo.append(float(bounds[0][a]) if i0 == 0 else float(lo[a]) + i0 * float(step[a]))
        box_hi.append(float(bounds[1][a]) if i1 == C else float(lo[a]) + i1 * float(step[a]))
    return box_lo, box_hi


def check_box(box, **refused):
    """``box=`` of an entry point: None, a SceneBox or a GridSpan (TypeError otherwise); with one, every keyword of ``refused``
    that is not None raises ValueError (``ts=``: the box places the positions)."""
    if box is None:
        return None
    if not isinstance(box, (SceneBox, GridSpan)):
        raise TypeError(f"box must be a utils.box.SceneBox or GridSpan (or None), got {type(box).__name__}")
    for name, v in refused.items():
        if v is not None:
            raise ValueError(f"box= places the sample positions itself: not together with {name}=")
    return box


def refuse_box(box, what):
    """The paths the scene box does not reach: refused before any launch and any RNG draw."""
    if box is not None:
        check_box(box)
        raise RuntimeError(f"box= serves the single-network renders and steps (render_nerf, render_view, evaluate, "
                           f"render_nerf_masked, train_step): not {what}")


def check_interval(N, tn, tf):
    """What nerf_amd_box_positions would refuse, raised before any draw."""
    if not 1 <= int(N) <= MAX_N:
        raise RuntimeError(f"the scene box places 1 <= N <= {MAX_N} samples per ray, got N = {N}")
    if not (math.isfinite(float(tn)) and math.isfinite(float(tf)) and float(tn) < float(tf)):
        raise ValueError(f"the scene box needs finite tn < tf, got tn = {tn!r}, tf = {tf!r}")


def place(box, rays, jit, flags, seed, ray_id0, N, tn, tf, want_span=False):
    """One launch of the box's placement (nerf_amd_box_positions, or nerf_amd_span_positions for a GridSpan) for settled
    jitter arguments -> (ts, span or None, hit or None)."""
    B, dev = rays.size(0), rays.device
    name, args = box.placement(dev)
    ts = torch.empty((B, N), dtype=torch.float32, device=dev)
    span = torch.empty((B, 2), dtype=torch.float32, device=dev) if want_span else None
    hit = torch.empty((B,), dtype=torch.int32, device=dev) if want_span else None
    tb = jitter.tbins(0, 1, N, dev, flags)
    _lib.launch(name, rays, jit, tb, flags, int(seed), int(ray_id0), *args, float(tn), float(tf), ts, span, hit, B, N, dev=dev)
    return ts, span, hit


def single(box, rays, N, tn, tf, *, u=None, device_rng=False, seed=0, ray_id0=0, shape_error=jitter.SHAPE_ERROR):
    """``box=`` of an entry point at the place where it settles its jitter: ``jitter.single`` for (u, device_rng), then the
    placement -> (ts, FLAG_TS_GIVEN, pending generator session or None), what the entry point's ``ts=`` path goes on with.
    The caller has run ``check_interval`` (and whatever else can raise) before: nothing here raises after the draw."""
    B = rays.size(0)
    jit, flags, pending = jitter.single(B, N, rays.device, u=u, device_rng=device_rng, shape_error=shape_error)
    try:
        ts = place(box, rays.detach().contiguous(), jit, flags, seed, ray_id0, N, tn, tf)[0]
    except BaseException:
        if pending is not None:
            pending.finish()
        raise
    return ts, _lib.FLAG_TS_GIVEN, pending
