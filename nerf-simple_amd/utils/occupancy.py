"""Empty-space skipping for the inference render: an occupancy grid and the masked render path.  Not in the reference.

    net = Nerf().cuda(); load_checkpoint(net, "model.pth")
    occ = occupancy_grid(net, 128, level=10.0, outside="empty")          # once per checkpoint
    pixels = render_view(net, pose, cam_params, device_rng=True, occupancy=occ)
    rgb, disp, alpha, acc, w = render_nerf(rays, net, 128, occupancy=occ)   # under torch.no_grad()

An ``OccupancyGrid`` is one bit per cell of a regular grid over ``bounds`` (R grid points per axis, the axes of
``mesh.grid_axes``, make R - 1 cells).  A sample of a ray is *live* iff the bit of the cell it falls in is set; a sample
outside the grid follows the grid's ``outside`` policy ('live': the grid does not speak for what it does not cover;
'empty': a bounded scene).  The masked render is the reference's ``volume_render`` over all N samples with the network's
output replaced by (0, 0, 0, -inf) at every dead sample -- which contributes exactly nothing -- and the network is only
evaluated at the live ones.  The semantics (packing, dilation rule, cell formula) are stated in include/nerf_amd.h and
restated in numpy by tests/occupancy_model.py.

Stages (csrc/occupancy.hip): mark (per-ray live masks) -> scan (offsets, live count) -> ONE host read of the live count
-> emit (compacted query points) -> the existing points-mode forward under the fp16 range guard -> masked composite.
Inference only, default network shape only, fp16 / bf16 / fp32.

Training with a grid: ``TrainingOccupancyGrid`` (a grid that is refreshed from the network while it trains) and
``training.render_nerf_masked`` / ``training.train_step(..., occupancy=)`` -- DESIGN.md section 13.

    occ = TrainingOccupancyGrid(128, outside="empty", device="cuda")
    for step in range(steps):
        if step >= warmup and step % 16 == 0:
            occ.update(net, level=-1.75)
        train_step(net, opt, rays, gt, 64, device_rng=True, seed=step, occupancy=occ)

Early ray termination (``EarlyTermination`` and ``render_terminated`` below): the samples hidden
behind what a ray has already hit are not evaluated either.

    term = EarlyTermination(eps=1e-3, slab=32)                           # no defaults: the caller states both
    pixels = render_view(net, pose, cam_params, device_rng=True, occupancy=occ, terminate=term)
    rgb, disp, alpha, acc, w = render_nerf(rays, net, 128, terminate=term)      # no grid: termination alone

The coarse + fine pair through ONE grid (``render_masked_pair`` below: ``render_hierarchical[_view](..., occupancy=)``;
``training.train_step_hierarchical(..., occupancy=)`` / ``training.GraphedMaskedHierarchicalTrainStep``) -- DESIGN.md
section 15.
"""
import numpy as np
import torch

from .. import _lib
from . import jitter
from .mesh import DEFAULT_BOUNDS, _resolution, density_grid, grid_axes

_POLICIES = ("live", "empty")
MAX_N = 768                             # samples per ray the mask layout and the masked compositor serve
MAX_N_TRAIN = 512                       # ... and the masked compositor's backward (the dense backward's own limit)


class MarkResult:
    """What ``OccupancyGrid.mark`` found: ``mask`` [B, ceil(N/64)] int64 (bit i & 63 of word i >> 6: sample i is live),
    ``offsets`` [B + 1] int64 (exclusive scan of the rays' live counts), ``live`` = offsets[B], a host int, and -- when
    asked for -- ``points`` [live, 6], the compacted query points the network is evaluated at."""

    def __init__(self, mask, offsets, live, B, N):
        self.mask, self.offsets, self.live, self.B, self.N = mask, offsets, live, B, N
        self.points = None

    @property
    def fraction(self):
        return self.live / max(1, self.B * self.N)


class OccupancyGrid:
    """Packed occupancy bits on the device.  Fields: ``words`` (int32 tensor, layout of include/nerf_amd.h),
    ``resolution`` (grid points per axis), ``bounds``, ``outside`` and ``cell_fraction`` (share of live cells).
    Build one with ``occupancy_grid`` (from a network), ``from_density`` (from a sigma volume) or ``from_mask``."""

    def __init__(self, words, resolution, bounds, outside):
        if outside not in _POLICIES:
            raise ValueError(f"outside must be 'live' or 'empty', got {outside!r}")
        self.words = words
        self.resolution = _resolution(resolution)
        self.bounds = (tuple(float(x) for x in bounds[0]), tuple(float(x) for x in bounds[1]))
        self.outside = outside
        self.lo, self.step = grid_axes(self.resolution, self.bounds)
        self.inv_step = (np.float32(1) / self.step).astype(np.float32)
        self.cell_fraction = self._count() / float(np.prod([r - 1 for r in self.resolution]))
        self.last_stats = None          # of the latest masked render through this grid

    # ---- construction -------------------------------------------------------------------------------------------------
    @classmethod
    def from_mask(cls, mask, bounds=DEFAULT_BOUNDS, *, outside="live"):
        """mask: bool (or any integer) device tensor [Cx, Cy, Cz], one entry per CELL (non-zero = live)."""
        if not torch.is_tensor(mask):
            raise AssertionError("mask needs to be a torch tensor")
        if not mask.is_cuda:
            raise RuntimeError(f"mask must live on the GPU (got a {mask.device} tensor); this package has no CPU path")
        if mask.dim() != 3:
            raise RuntimeError("from_mask expects a 3-D cell mask [Cx, Cy, Cz]")
        R = _resolution(tuple(int(c) + 1 for c in mask.shape))
        cells = (mask != 0).to(torch.uint8).contiguous()
        lib = _lib.lib()
        words = torch.empty(_grid_words(lib, R), dtype=torch.int32, device=mask.device)
        _lib.launch("nerf_amd_occupancy_from_mask", cells, *R, words, dev=mask.device)
        return cls(words, R, bounds, outside)

    @classmethod
    def from_density(cls, sigma, level, bounds=DEFAULT_BOUNDS, dilate=1, outside="live"):
        """sigma: float32 device volume [Rx, Ry, Rz] of raw sigma on the grid POINTS (``mesh.density_grid``).  A cell is
        dead iff every corner of every cell within ``dilate`` cells of it has sigma <= level (NaN makes it live)."""
        _lib.require_cuda_f32(sigma, "sigma")
        if sigma.dim() != 3:
            raise RuntimeError("from_density expects a 3-D volume [Rx, Ry, Rz]")
        if int(dilate) != dilate or dilate < 0:
            raise ValueError(f"dilate must be a non-negative integer, got {dilate!r}")
        R = _resolution(tuple(sigma.shape))
        sigma = sigma.detach().contiguous()
        lib = _lib.lib()
        words = torch.empty(_grid_words(lib, R), dtype=torch.int32, device=sigma.device)
        _lib.launch("nerf_amd_occupancy_from_density", sigma, *R, float(level), int(dilate), words, dev=sigma.device)
        return cls(words, R, bounds, outside)

    # ---- inspection ---------------------------------------------------------------------------------------------------
    def cells(self):
        """The bits unpacked: a bool device tensor [Cx, Cy, Cz]."""
        C = [r - 1 for r in self.resolution]
        wz = (C[2] + 31) // 32
        shifts = torch.arange(32, dtype=torch.int32, device=self.words.device)
        b = (self.words.view(C[0], C[1], wz, 1) >> shifts) & 1
        return b.view(C[0], C[1], wz * 32)[:, :, :C[2]].bool()

    def _count(self):
        shifts = torch.arange(32, dtype=torch.int32, device=self.words.device)
        return int(((self.words.view(-1, 1) >> shifts) & 1).sum())          # padding bits are zero; one host read

    def mark(self, rays, N, tn=2, tf=6, *, u=None, ts=None, device_rng=False, seed=0, ray_id0=0, points=False):
        """Which samples a render of ``rays`` with these arguments evaluates: a ``MarkResult`` (with ``points=True``
        also the compacted query points).  Jitter sources as ``render_nerf`` (u / ts explicit, the counter RNG, default
        one reference ``torch.rand(B, N)``).  One host synchronisation."""
        B, N = _lib.require_rays(rays), int(N)
        jit, flags, pending = jitter.single(B, N, rays.device, u=u, ts=ts, device_rng=device_rng)
        try:
            rays, tbins = rays.detach().contiguous(), jitter.tbins(tn, tf, N, rays.device, flags)
            m = _mark(self, rays, jit, tbins, flags, seed, ray_id0, N)
            if points:
                m.points = _points(m, rays, jit, tbins, flags, seed, ray_id0)
            return m
        finally:
            if pending is not None:
                pending.finish()


def softplus_level(level):
    """softplus(level) as a float32 (beta = 1, identity above 20, numpy's float32 exp / log1p): the threshold a
    ``TrainingOccupancyGrid`` compares its density-unit state volume with, for a ``level`` given in raw-sigma units."""
    x = np.float32(level)
    with np.errstate(over="ignore"):
        return x if x > np.float32(20) else np.log1p(np.exp(x, dtype=np.float32), dtype=np.float32)


class TrainingOccupancyGrid(OccupancyGrid):
    """An occupancy grid that follows a network while it trains.  It starts with every cell live and
    keeps ``state``, a float32 volume [Rx, Ry, Rz] on the grid points: a decayed running maximum of the density
    softplus(sigma) seen at each point, zero at first.  ``update`` refreshes the bits in place, so the grid object handed
    to ``training.train_step(..., occupancy=)`` / ``training.render_nerf_masked`` stays the same; being an
    ``OccupancyGrid`` it also serves the inference renders."""

    def __init__(self, resolution, bounds=DEFAULT_BOUNDS, *, outside="empty", device):
        R = _resolution(resolution)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"the occupancy grid must live on the GPU (got {device}); this package has no CPU path")
        cells = torch.ones(tuple(r - 1 for r in R), dtype=torch.bool, device=device)
        words = OccupancyGrid.from_mask(cells, bounds, outside=outside).words
        super().__init__(words, R, bounds, outside)
        self.state = torch.zeros(R, dtype=torch.float32, device=device)
        self.updates = 0

    def update(self, net, level, *, decay=0.95, dilate=1, precision=None):
        """state <- max(state * decay, softplus(sigma of ``net`` on the grid)); bits <- state against softplus(level) with
        the corner / dilation rule of ``from_density``, written into the same ``words`` tensor; ``cell_fraction``
        refreshed (one host read).  level: raw-sigma units, no default.  Runs under ``torch.no_grad()``."""
        if int(dilate) != dilate or dilate < 0:
            raise ValueError(f"dilate must be a non-negative integer, got {dilate!r}")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"decay must lie in [0, 1], got {decay!r}")
        with torch.no_grad():
            sigma = density_grid(net, self.resolution, self.bounds, precision=precision)
        if sigma.device != self.state.device:
            raise RuntimeError(f"the occupancy grid lives on {self.state.device}, the network on {sigma.device}")
        dev = self.state.device
        _lib.launch("nerf_amd_occupancy_decay_max", self.state, sigma, float(decay), self.state.numel(), dev=dev)
        _lib.launch("nerf_amd_occupancy_from_density", self.state, *self.resolution, float(softplus_level(level)), int(dilate),
                    self.words, dev=dev)
        self.cell_fraction = self._count() / float(np.prod([r - 1 for r in self.resolution]))
        self.updates += 1
        return self


def check_trainable(occupancy, net, rays, N, precision=None):
    """The preconditions of ``training.render_nerf_masked``; raises before any jitter is drawn."""
    from .nets import Nerf
    if not isinstance(occupancy, OccupancyGrid):
        raise TypeError("occupancy must be an OccupancyGrid (utils/occupancy.py)")
    if not (isinstance(net, Nerf) and net._fused_ok()):
        raise RuntimeError("masked training (occupancy=) serves the default Nerf(10, 4, 256) only: other network sizes and "
                           "foreign nets are not supported; train without occupancy")
    if _lib.precision_of(net, precision) == _lib.F32:
        raise RuntimeError("masked training (occupancy=) runs the fused bf16 training kernels: precision='fp32' modules are "
                           "not supported; build the module with precision='bf16' or 'fp16', or train without occupancy")
    if rays.requires_grad:
        raise RuntimeError("masked training (occupancy=) gives no gradients to the rays; detach them, or render without "
                           "occupancy")
    if int(N) > MAX_N_TRAIN:
        raise RuntimeError(f"masked training serves 1 <= N <= {MAX_N_TRAIN} samples per ray, got N = {N}")


def _grid_words(lib, R):
    n = int(lib.nerf_amd_occupancy_grid_words(*R))
    if n < 0:
        raise RuntimeError(f"occupancy grid: unsupported resolution {R}")
    return n


def occupancy_grid(net, resolution=128, level=None, bounds=DEFAULT_BOUNDS, *, dilate=1, outside="live", precision=None):
    """``OccupancyGrid.from_density(density_grid(net, resolution, bounds), level, bounds, dilate, outside)``.

    level is in raw-sigma units, like ``extract_mesh``'s, and has NO default: what a level costs in image quality depends
    on the trained scene, so the caller states it.  Corner sampling cannot see what the network
    does inside a cell, which is why ``dilate`` defaults to 1."""
    if level is None:
        raise TypeError("occupancy_grid() needs a level (raw-sigma units): there is no default, see DESIGN.md section 12")
    sigma = density_grid(net, resolution, bounds, precision=precision)
    return OccupancyGrid.from_density(sigma, level, bounds, dilate, outside)


def check_renderable(occupancy, net, rays_require_grad):
    """The masked render's preconditions; raises before any jitter is drawn."""
    from .nets import Nerf
    if not isinstance(occupancy, OccupancyGrid):
        raise TypeError("occupancy must be an OccupancyGrid (utils/occupancy.py)")
    if not (isinstance(net, Nerf) and net._fused_ok()):
        raise RuntimeError("the masked render (occupancy=) serves the default Nerf(10, 4, 256) only: other network sizes "
                           "and foreign nets are not supported; render without occupancy")
    if torch.is_grad_enabled() and (rays_require_grad or any(p.requires_grad for p in net.parameters())):
        raise RuntimeError("the masked render (occupancy=) is inference only: call it under torch.no_grad()")


def _mark(occ, rays, jit, tbins, flags, seed, ray_id0, N):
    B, dev = rays.size(0), rays.device
    _lib.require_same_device("occupancy grid", occ.words, dev)
    lib = _lib.lib()
    nwords = int(lib.nerf_amd_occupancy_mask_words(B, N))
    if nwords < 0:
        raise RuntimeError(f"the masked render serves 1 <= N <= {MAX_N} samples per ray, got N = {N}")
    mask = torch.empty((B, (N + 63) // 64), dtype=torch.int64, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    ws = _lib.workspace(lib.nerf_amd_occupancy_workspace_bytes(B), dev)
    mflags = flags | (_lib.FLAG_OUTSIDE_EMPTY if occ.outside == "empty" else 0)
    _lib.launch("nerf_amd_occupancy_mark", rays, jit, tbins, mflags, int(seed), int(ray_id0), occ.words, *occ.resolution,
                _lib.host_f32x3(occ.lo), _lib.host_f32x3(occ.inv_step), mask, offsets, None, ws, B, N, dev=dev)
    live = int(offsets[B])              # the one host synchronisation of a masked render
    return MarkResult(mask, offsets, live, B, N)


def _points(m, rays, jit, tbins, flags, seed, ray_id0):
    """The compacted query points [P', 6] of a MarkResult."""
    dev = rays.device
    pts = torch.empty((m.live, 6), dtype=torch.float32, device=dev)
    if m.live:
        _lib.launch("nerf_amd_occupancy_points", rays, jit, tbins, flags, int(seed), int(ray_id0), m.mask, m.offsets, pts,
                    m.live, m.B, m.N, dev=dev)
    return pts


def sample_positions(rays, jit, tbins, flags, seed, ray_id0, N):
    """ts [B, N] of these jitter arguments, as nerf_amd_query_points forms them (given positions come back as they are)."""
    if flags & _lib.FLAG_TS_GIVEN:
        return jit
    from .rendering import _query_points
    return _query_points(rays, jit, tbins, flags, seed, ray_id0, N)[1]


def _masked_composite(raw, head, m, outputs, pixels, st):
    """The masked compositor on the live rows ``raw`` (None: no live row) of a MarkResult, enqueued on ``st``: pixels [B, 4],
    or the 5-tuple.  ``head`` = (rays, jitter, tbins, flags, seed, ray_id0)."""
    from .rendering import _five_outputs, _per_sample
    B, N, dev = m.B, m.N, head[0].device
    chead = (raw, *head, m.mask, m.offsets)
    if pixels:
        px = torch.empty((B, 4), dtype=torch.float32, device=dev)
        _lib.launch("nerf_amd_volume_render_masked_pixels", *chead, px, B, N, stream=st)
        return px
    rgb, disp, alpha, acc, w = _five_outputs(B, N, outputs, dev)
    _lib.launch("nerf_amd_volume_render_masked", *chead, rgb, disp, alpha, acc, w, B, N, stream=st)
    return rgb, disp, _per_sample(alpha, N), acc, _per_sample(w, N)


def _masked_pass(occ, rays, N, tbins, jit, flags, seed, ray_id0, outputs, pixels, mark=None):
    """mark + emit of one masked pass, now (one host read) -> (MarkResult, stats, launch); ``launch(code, image)`` enqueues
    the network on the live points and the masked compositor and returns the 5-tuple, or pixels [B, 4].  ``mark``: the
    ready MarkResult of these positions (the masked guided placement produces it with them): no mark is launched."""
    B, dev = rays.size(0), rays.device
    m = _mark(occ, rays, jit, tbins, flags, seed, ray_id0, N) if mark is None else mark
    pts = _points(m, rays, jit, tbins, flags, seed, ray_id0)
    stats = {"rays": B, "samples": B * N, "live": m.live, "network_launches": 0}

    def launch(code, image):
        raw = None
        with torch.cuda.device(dev):          # one guard and one stream lookup for the pass's two launches
            st = _lib.stream_ptr(dev)
            if m.live:
                raw = torch.empty((m.live, 4), dtype=torch.float32, device=dev)
                _lib.launch("nerf_amd_mlp_forward", pts, image, raw, m.live, code, stream=st)
                stats["network_launches"] += 1
            return _masked_composite(raw, (rays, jit, tbins, flags, int(seed), int(ray_id0)), m, outputs, pixels, st)

    return m, stats, launch


def render_masked(occ, rays, net, N, tbins, jit, flags, seed, ray_id0, code, outputs, pixels=False):
    """The body of ``render_nerf(..., occupancy=occ)`` / ``render_view(..., occupancy=occ)`` once rays, jitter and
    precision are settled.  Returns the 5-tuple, or pixels [B, 4] with ``pixels=True``."""
    return _render_pass(occ, rays, net, code, _masked_pass(occ, rays, N, tbins, jit, flags, seed, ray_id0, outputs, pixels))


def _render_marked(occ, rays, net, ts, mark, code, outputs, pixels=False):
    """``render_masked`` on given positions ``ts`` [B, N] whose MarkResult through ``occ`` is already there (the masked guided
    placement, ``ProposalVolume.sample(..., occupancy=occ, return_mark=True)``): emit, network, masked compositor."""
    N = ts.size(1)
    return _render_pass(occ, rays, net, code,
                        _masked_pass(occ, rays, N, None, ts, _lib.FLAG_TS_GIVEN, 0, 0, outputs, pixels, mark=mark))


def _render_pass(occ, rays, net, code, masked_pass):
    from .nets import guarded_launch
    m, stats, launch = masked_pass
    occ.last_stats = stats
    if rays.size(0) == 0 or m.live == 0:
        # nothing to evaluate: no network launch, hence nothing for the range guard to look at
        return launch(code, None)
    return guarded_launch([net], code, lambda code, packed: launch(code, packed[0]))


SLABS = (16, 32, 64)                    # samples per slab: a slab never straddles a 64-sample chunk of the compositor


class EarlyTermination:
    """Early ray termination for the inference renders: ``render_nerf(..., terminate=term)`` /
    ``render_view(..., terminate=term)``, with or without ``occupancy=``.  A ray's samples are evaluated in slabs of ``slab``
    sample indices (16, 32 or 64); before each slab the ray's transmittance T over the rows evaluated so far is formed in
    the compositor's arithmetic, and a ray with T < ``eps`` evaluates nothing more.  The result is the masked render under
    the evaluated mask (include/nerf_amd.h, "terminated render"): each rgb channel moves by less than eps max|c| over the
    dropped samples and acc by less than eps.  Neither argument has a default: what an eps costs in image quality and
    which slab is fastest depend on the scene, so the caller states both.

    After a render: ``last_stats`` (a plain dict: {'rays', 'samples', 'live', 'evaluated', 'terminated_rays', 'slabs_run',
    'network_launches', 'host_reads'}; 'terminated_rays' = rays with T < eps at the last check, which comes back with the
    loop's last host read; every figure describes the pass that produced the outputs -- after an fp16 overflow the repeat
    with bf16 operands, whose counters start afresh), ``transmittance`` [B, K] (the T_k; column 0 is 1; columns the loop did
    not reach repeat the last one formed) and ``evaluated_mask`` [B, ceil(N / 64)] int64 (the layout of ``MarkResult.mask``)."""

    def __init__(self, eps, slab):
        if isinstance(slab, bool) or not isinstance(slab, (int, np.integer)) or int(slab) not in SLABS:
            raise ValueError(f"slab must be 16, 32 or 64 samples, got {slab!r}")
        try:
            e = np.float32(eps)
        except (TypeError, ValueError):
            raise ValueError(f"eps must be a number in (0, 1), got {eps!r}") from None
        if not (e > 0 and e < 1):
            raise ValueError(f"eps must lie in (0, 1) as a float32, got {eps!r}")
        self.eps, self.slab = float(e), int(slab)
        self.last_stats = None
        self.transmittance = None
        self.evaluated_mask = None


_ALL_LIVE = {}


def all_live_grid(device):
    """The one-cell grid termination runs on when the caller has none: every sample is live (``outside='live'``)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _ALL_LIVE:
        _ALL_LIVE[device] = OccupancyGrid.from_mask(torch.ones((1, 1, 1), dtype=torch.bool, device=device), DEFAULT_BOUNDS,
                                                    outside="live")
    return _ALL_LIVE[device]


def check_terminable(terminate, occupancy, net, rays_require_grad):
    """The terminated render's preconditions (the masked render's, and an ``EarlyTermination``); raises before any jitter
    is drawn."""
    from .nets import Nerf
    if not isinstance(terminate, EarlyTermination):
        raise TypeError("terminate must be an EarlyTermination (utils/occupancy.py)")
    if occupancy is not None:
        return check_renderable(occupancy, net, rays_require_grad)
    if not (isinstance(net, Nerf) and net._fused_ok()):
        raise RuntimeError("the terminated render (terminate=) serves the default Nerf(10, 4, 256) only: other network sizes "
                           "and foreign nets are not supported; render without terminate")
    if torch.is_grad_enabled() and (rays_require_grad or any(p.requires_grad for p in net.parameters())):
        raise RuntimeError("the terminated render (terminate=) is inference only: call it under torch.no_grad()")


def render_terminated(term, occ, rays, net, N, tbins, jit, flags, seed, ray_id0, code, outputs, pixels=False):
    """The body of ``render_nerf(..., terminate=term)`` / ``render_view(..., terminate=term)``: ``render_masked`` with the
    network run slab by slab.  mark (one host read of P'0) -> raw0 [P'0, 4] filled with (0, 0, 0, -inf) -> advance selects
    slab 0 -> per slab: read the two counts (one host read), stop if nothing remains, emit the slab's points, the network on
    them (nothing when the slab is empty), advance (retire the rows into raw0, T, select the next slab) -> the masked
    compositor on (raw0, M0): at most K + 1 host reads.  ``occ`` None: the all-live grid."""
    from .nets import guarded_launch
    B, dev = rays.size(0), rays.device
    if occ is None:
        occ = all_live_grid(dev)
    S, K, W = term.slab, (N + term.slab - 1) // term.slab, (N + 63) // 64
    m = _mark(occ, rays, jit, tbins, flags, seed, ray_id0, N)          # M0; raises for N > MAX_N
    trans = torch.ones((B, K), dtype=torch.float32, device=dev)
    evaluated_mask = torch.zeros((B, W), dtype=torch.int64, device=dev)
    stats = {"rays": B, "samples": B * N, "live": m.live, "evaluated": 0, "terminated_rays": 0, "slabs_run": 0,
             "network_launches": 0, "host_reads": 1}
    term.last_stats, term.transmittance, term.evaluated_mask = stats, trans, evaluated_mask
    occ.last_stats = stats
    masks = [torch.empty((B, W), dtype=torch.int64, device=dev) for _ in range(2)]
    offs = [torch.empty(B + 1, dtype=torch.int64, device=dev) for _ in range(2)]
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = _lib.workspace(_lib.lib().nerf_amd_termination_workspace_bytes(B), dev)
    dead_row = torch.tensor([0.0, 0.0, 0.0, -np.inf], dtype=torch.float32, device=dev) if B else None
    head = (rays, jit, tbins, flags, int(seed), int(ray_id0))

    def advance(raw, cur, rows, s0, s1, s2, raw0, st):
        _lib.launch("nerf_amd_termination_advance", raw, masks[cur] if raw is not None else None,
                    offs[cur] if raw is not None else None, rows, *head, m.mask, m.offsets, raw0, m.live, term.eps, S, s0, s1, s2,
                    trans, masks[1 - cur], offs[1 - cur], totals, ws, B, N, stream=st)

    def launch(code, image):
        raw0 = None
        with torch.cuda.device(dev):          # one guard and one stream lookup for the slab loop (host reads between its launches)
            st = _lib.stream_ptr(dev)
            if B:
                raw0 = dead_row.repeat(max(m.live, 1), 1)
                evaluated_mask.zero_()
                # the counters of THIS pass (a repeat under the range guard starts afresh; the mark's read is kept)
                stats.update(evaluated=0, terminated_rays=0, slabs_run=0, network_launches=0, host_reads=1)
                cur = 1
                advance(None, cur, 0, 0, 0, min(S, N), raw0, st)               # T_0 = 1, selects slab 0 into masks[0]
                cur = 0
                for k in range(K):
                    # one host read per slab: the two counts and, with them, the rays terminated at this check (column k is
                    # final: it was formed before slab k is evaluated)
                    count, remaining, gone = torch.cat((totals, (trans[:, k] < term.eps).sum().view(1))).tolist()
                    stats["host_reads"] += 1
                    stats["terminated_rays"] = gone
                    if remaining == 0:
                        if k + 1 < K:
                            trans[:, k + 1:] = trans[:, k:k + 1]
                        break
                    raw = None
                    if count:
                        pts = torch.empty((count, 6), dtype=torch.float32, device=dev)
                        _lib.launch("nerf_amd_occupancy_points", *head, masks[cur], offs[cur], pts, count, B, N, stream=st)
                        raw = torch.empty((count, 4), dtype=torch.float32, device=dev)
                        _lib.launch("nerf_amd_mlp_forward", pts, image, raw, count, code, stream=st)
                        stats["network_launches"] += 1
                        stats["evaluated"] += count
                        evaluated_mask.bitwise_or_(masks[cur])
                    s1 = min(k * S + S, N)
                    advance(raw, cur, count, k * S, s1, min(s1 + S, N), raw0, st)
                    stats["slabs_run"] += 1
                    cur = 1 - cur
            return _masked_composite(raw0 if m.live else None, head, m, outputs, pixels, st)

    if B == 0 or m.live == 0:
        # nothing to evaluate: no network launch, hence nothing for the range guard to look at
        return launch(code, None)
    return guarded_launch([net], code, lambda code, packed: launch(code, packed[0]))


def render_masked_pair(occ, rays, net_c, net_f, Nc, Nf, tbins, jit_c, flags, u_f, device_rng, seed, ray_id0, code, pixels=False):
    """The body of ``render_hierarchical(..., occupancy=occ)`` / ``render_hierarchical_view(..., occupancy=occ)``: the
    masked coarse pass -> ``sample_pdf`` on its weights (0 at a dead sample) -> the masked pass of ``net_f`` on the merged
    positions through the same grid, both passes at ONE precision under one range guard.  Two host reads (one live count
    per pass).  Returns (fine 5-tuple or pixels [B, 4], coarse 5-tuple, ts_f); ``occ.last_stats`` reports both passes."""
    from .nets import guarded_launch
    from .rendering import ALL_OUTPUTS, sample_pdf
    ts_c = sample_positions(rays, jit_c, tbins, flags, seed, ray_id0, Nc)
    _, stats_c, launch_c = _masked_pass(occ, rays, Nc, tbins, jit_c, flags, seed, ray_id0, ALL_OUTPUTS, False)

    def launch(code, packed):
        coarse = launch_c(code, packed[0])
        ts_f = sample_pdf(ts_c, coarse[4], Nf, u=u_f, device_rng=device_rng, seed=seed, ray_id0=ray_id0)
        _, stats_f, launch_f = _masked_pass(occ, rays, Nc + Nf, None, ts_f, _lib.FLAG_TS_GIVEN, 0, 0, ALL_OUTPUTS, pixels)
        fine = launch_f(code, packed[-1])
        stats = {k: stats_c[k] + stats_f[k] for k in ("samples", "live", "network_launches")}
        stats.update(rays=stats_c["rays"], coarse=stats_c, fine=stats_f)
        occ.last_stats = stats
        return fine, coarse, ts_f

    # one precision for both passes: if either network left the fp16 range, both render with bf16 operands
    return guarded_launch([net_c] if net_f is net_c else [net_c, net_f], code, launch)
