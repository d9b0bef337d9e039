"""Grid-guided fine sampling: the importance samples of a ray placed from a sigma volume on a grid instead of a coarse
network.  Not in the reference; DESIGN.md section 21, semantics in include/nerf_amd.h ("grid-guided fine sampling").

    prop = ProposalVolume(128, device="cuda")                  # all -inf: nothing known yet, uniform placement
    prop.update(net)                                           # sigma of ``net`` on the grid, in place (about 1.4 ms at 128^3)
    pixels = render_guided_view(net, pose, cam_params, 64, 128, prop, device_rng=True)
    loss = train_step_guided(net, opt, rays, gt, 64, 128, prop, device_rng=True, seed=step)

``ProposalVolume.sample`` is ONE kernel (csrc/guided_sample.hip): the Nc coarse positions of a ray, the maximum of the
volume over the 8 corners of each position's cell (the occupancy grid's cell rule; -inf outside the grid, NaN corners
skipped), the compositor's weights of raw = (0, 0, 0, value), and ``sample_pdf`` on those weights -> ts [B, Nc + Nf].  By
definition it equals nerf_amd_query_points -> look-up -> nerf_amd_volume_render_rays -> nerf_amd_sample_pdf bit for bit;
tests/guided_model.py restates the look-up and the composition in numpy.  The positions carry no gradient.

With ``occupancy=`` (an ``OccupancyGrid``) the sampler is the masked guided placement (csrc/guided_masked.hip, DESIGN.md
section 24): dead coarse samples weigh nothing and the merged positions come back marked, so ``render_guided``,
``render_guided_view`` and ``train_step_guided`` evaluate the network at the live ones only.

There is no default for the resolution or for how often ``update`` runs: the caller states both.
"""
import numpy as np
import torch

from .. import _lib
from . import jitter
from .mesh import DEFAULT_BOUNDS, _resolution, _warn_if_out_of_range, density_grid, grid_axes

MIN_NC, MAX_NC, MAX_TOTAL = 3, 256, 512           # the sampler's sizes (csrc/sample_pdf_device.h)


def check_sizes(Nc, Nf):
    if int(Nc) != Nc or int(Nf) != Nf or Nc < MIN_NC or Nc > MAX_NC or Nf < 0 or Nc + Nf > MAX_TOTAL:
        raise ValueError(f"guided sampling needs {MIN_NC} <= Nc <= {MAX_NC}, Nf >= 0 and Nc + Nf <= {MAX_TOTAL} "
                         f"(got Nc={Nc}, Nf={Nf})")
    return int(Nc), int(Nf)


class ProposalVolume:
    """A float32 volume ``sigma`` [Rx, Ry, Rz] of raw sigma on the grid points of ``mesh.grid_axes(resolution, bounds)``,
    and the sampler that reads it.  A new volume holds -inf everywhere: every ray gets the sampler's uniform placement
    until ``update`` has run.  ``sigma`` is written in place, so its address is stable (a captured graph may bake it in);
    do not replace the tensor."""

    def __init__(self, resolution, bounds=DEFAULT_BOUNDS, *, device):
        R = _resolution(resolution)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"the proposal volume must live on the GPU (got {device}); this package has no CPU path")
        self._init(torch.full(R, float("-inf"), dtype=torch.float32, device=device), R, bounds)

    def _init(self, sigma, R, bounds):
        self.sigma = sigma
        self.resolution = R
        self.bounds = (tuple(float(x) for x in bounds[0]), tuple(float(x) for x in bounds[1]))
        self.lo, self.step = grid_axes(R, self.bounds)
        self.inv_step = (np.float32(1) / self.step).astype(np.float32)
        self._h_lo, self._h_inv_step = _lib.host_f32x3(self.lo), _lib.host_f32x3(self.inv_step)
        self.updates = 0

    @classmethod
    def from_sigma(cls, volume, bounds=DEFAULT_BOUNDS):
        """volume: float32 device tensor [Rx, Ry, Rz] of raw sigma on the grid points (``mesh.density_grid``'s output); it is
        used as it is when contiguous (no copy), so later in-place writes to it are seen."""
        _lib.require_cuda_f32(volume, "volume")
        if volume.dim() != 3:
            raise RuntimeError("from_sigma expects a 3-D volume [Rx, Ry, Rz]")
        self = cls.__new__(cls)
        self._init(volume.detach().contiguous(), _resolution(tuple(volume.shape)), bounds)
        return self

    def update(self, net, precision=None):
        """sigma <- raw sigma of ``net`` on the grid (``mesh.density_grid``, bit for bit), written IN PLACE.  fp16 / bf16 run
        the sigma-only kernel straight into ``sigma`` under the range guard of the 16-bit kernels; fp32 evaluates the grid
        in chunks and copies.  Default network shape only.  Runs under ``torch.no_grad()``."""
        from .nets import Nerf, guarded_launch
        if not (isinstance(net, Nerf) and net._fused_ok()):
            raise RuntimeError("guided sampling serves the default Nerf(10, 4, 256) only: other network sizes and foreign "
                               "nets are not supported")
        dev = self.sigma.device
        if next(net.parameters()).device != dev:
            raise RuntimeError(f"the proposal volume lives on {dev}, the network on {next(net.parameters()).device}")
        code = _lib.precision_of(net, precision)
        R = self.resolution
        _warn_if_out_of_range(R, self.lo, self.step)
        h_lo, h_step = _lib.host_f32x3(self.lo), _lib.host_f32x3(self.step)

        def launch(code, packed):
            if code == _lib.F32:
                self.sigma.copy_(density_grid(net, R, self.bounds, precision="fp32"))
            else:
                _lib.launch("nerf_amd_density_grid", h_lo, h_step, R[0], R[1], R[2], packed[0], code, self.sigma, dev=dev)
            return self.sigma

        with torch.no_grad():
            guarded_launch([net], code, launch)
        self.updates += 1
        return self

    # ---- the sampler ------------------------------------------------------------------------------------------------------
    def _launch(self, rays, jit, tbins, flags, seed, ray_id0, u_f, ts_out, sigma_c, w_c, B, Nc, Nf):
        """Enqueue nerf_amd_sample_pdf_volume on the current stream of the volume's device (no allocation, no sync)."""
        _lib.launch("nerf_amd_sample_pdf_volume", rays, jit, tbins, flags, int(seed), int(ray_id0), self.sigma,
                    *self.resolution, self._h_lo, self._h_inv_step, u_f, ts_out, sigma_c, w_c, B, Nc, Nf, dev=self.sigma.device)

    def _launch_masked(self, occ, rays, jit, tbins, flags, seed, ray_id0, u_f, ts_out, sigma_c, w_c, mask, offsets, live, ws,
                       B, Nc, Nf):
        """Enqueue nerf_amd_sample_pdf_volume_masked (placement + mark + scan through ``occ``) likewise."""
        mflags = flags | (_lib.FLAG_OUTSIDE_EMPTY if occ.outside == "empty" else 0)
        _lib.launch("nerf_amd_sample_pdf_volume_masked", rays, jit, tbins, mflags, int(seed), int(ray_id0), self.sigma,
                    *self.resolution, self._h_lo, self._h_inv_step, occ.words, *occ.resolution, _lib.host_f32x3(occ.lo),
                    _lib.host_f32x3(occ.inv_step), u_f, ts_out, sigma_c, w_c, mask, offsets, live, ws, B, Nc, Nf,
                    dev=self.sigma.device)

    def check(self, rays, Nc, Nf, u_c=None, ts_c=None, u_f=None, device_rng=False, *, occupancy=None):
        """The preconditions of ``sample``; raises before any jitter is drawn.  -> (B, Nc, Nf)"""
        if occupancy is not None:
            from .occupancy import OccupancyGrid
            if not isinstance(occupancy, OccupancyGrid):
                raise TypeError("occupancy must be an OccupancyGrid (utils/occupancy.py)")
        Nc, Nf = check_sizes(Nc, Nf)
        B = _lib.require_rays(rays)
        if torch.is_grad_enabled() and rays.requires_grad:
            raise RuntimeError("guided sampling gives no gradients to the rays; detach them")
        if not (torch.is_tensor(self.sigma) and self.sigma.is_cuda and self.sigma.dtype == torch.float32
                and self.sigma.is_contiguous() and tuple(self.sigma.shape) == self.resolution):
            raise RuntimeError("ProposalVolume.sigma must stay the contiguous float32 device volume it was built with")
        _lib.require_same_device("proposal volume", self.sigma, rays.device)
        if u_c is not None and ts_c is not None:
            raise ValueError("give u_c or ts_c, not both")
        if device_rng and u_c is not None:
            raise ValueError("device_rng=True draws the coarse jitter on the device: it cannot be combined with u_c")
        if device_rng and u_f is not None:
            raise ValueError("device_rng=True draws the fine jitter on the device: it cannot be combined with u_f")
        for name, t_, n in (("u_c", u_c, Nc), ("ts_c", ts_c, Nc), ("u_f", u_f, Nf)):
            _lib.require_shape(t_, name, (B, n))
        if occupancy is not None:
            _lib.require_same_device("occupancy grid", occupancy.words, rays.device)
        return B, Nc, Nf

    def sample(self, rays, Nc, Nf, tn=2, tf=6, *, u_c=None, ts_c=None, u_f=None, device_rng=False, seed=0, ray_id0=0,
               return_weights=False, occupancy=None, return_mark=False):
        """ts [B, Nc + Nf]: the Nc coarse positions of ``render_nerf`` for these jitter arguments merged with Nf importance
        samples of the volume's weights, sorted.  Coarse jitter: ``u_c`` [B, Nc] / ``ts_c`` [B, Nc] explicit, or
        ``device_rng=True`` (counter RNG keyed by ``seed``, ``ray_id0``); fine jitter: ``u_f`` [B, Nf], or the counter RNG
        with ``device_rng=True`` (``sample_pdf``'s key).  Default: ``render_hierarchical``'s draws, ``torch.rand(B, Nc)`` then
        ``torch.rand(B, Nf)`` from torch's CPU generator, continued on the device.  return_weights: also the looked-up
        values and the weights, (ts, sigma_c [B, Nc], w_c [B, Nc]).  No host synchronisation; every refusal happens before
        anything is drawn.

        occupancy: an ``OccupancyGrid`` -- the masked guided placement (one entry point,
        nerf_amd_sample_pdf_volume_masked): a coarse sample in a dead cell of the grid weighs exactly 0, so the new samples
        gather in live cells, and the merged positions are marked through the same grid.  ``sigma_c`` is then the value
        after that masking (-inf at a dead coarse sample).  return_mark (needs ``occupancy``): the ``MarkResult`` of the
        merged positions (utils/occupancy.py) comes back as the last element; reading its live count is the call's one host
        synchronisation."""
        if return_mark and occupancy is None:
            raise ValueError("return_mark=True needs an occupancy grid")
        B, Nc, Nf = self.check(rays, Nc, Nf, u_c, ts_c, u_f, device_rng, occupancy=occupancy)
        dev = rays.device
        rays = rays.detach().contiguous()
        # ``check`` has refused what this sampler refuses (u_c / u_f with device_rng, u_c with ts_c) and looked at every shape
        jit, flags, pending = jitter.single(B, Nc, dev, u=u_c, ts=ts_c, device_rng=device_rng, names=("u_c", "ts_c"),
                                            shape_error=None)
        if pending is not None:
            pending.finish()
        if device_rng:
            flags |= _lib.FLAG_DEVICE_RNG             # with ts_c given too: the fine samples still come from the counter RNG
        # this entry point's own rule (section 31): nothing is drawn for Nf == 0 and u_f stays None
        u_f, _, pending = jitter.single(B, Nf, dev, u=u_f, device_rng=device_rng or Nf == 0, names=("u_f", None),
                                        shape_error=None)
        if pending is not None:
            pending.finish()
        tbins = jitter.tbins(tn, tf, Nc, dev, flags)
        ts = torch.empty((B, Nc + Nf), dtype=torch.float32, device=dev)
        sigma_c = w_c = None
        if return_weights:
            sigma_c = torch.empty((B, Nc), dtype=torch.float32, device=dev)
            w_c = torch.empty((B, Nc), dtype=torch.float32, device=dev)
        if occupancy is None:
            self._launch(rays, jit, tbins, flags, seed, ray_id0, u_f, ts, sigma_c, w_c, B, Nc, Nf)
            return (ts, sigma_c, w_c) if return_weights else ts
        from .occupancy import MarkResult
        N = Nc + Nf
        mask = torch.empty((B, (N + 63) // 64), dtype=torch.int64, device=dev)
        offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
        ws = _lib.workspace(_lib.lib().nerf_amd_occupancy_workspace_bytes(B), dev)
        self._launch_masked(occupancy, rays, jit, tbins, flags, seed, ray_id0, u_f, ts, sigma_c, w_c, mask, offsets, None, ws,
                            B, Nc, Nf)
        out = (ts, sigma_c, w_c) if return_weights else (ts,)
        if return_mark:
            out += (MarkResult(mask, offsets, int(offsets[B]), B, N),)          # the one host synchronisation
        return out if len(out) > 1 else ts
