"""Camera optimiser: one learnable pose correction per training image, trained beside the network (not in the reference,
whose poses are exact by construction; BARF, NeRF-- and nerfstudio's camera optimiser learn such a correction).

Image m of M has the stored pose [R0 | t0] and the correction ``xi[m] = (w, tau)``: R = exp([w]x) R0, t = t0 + tau
(csrc/camera_device.h).  ``CameraRefinement.rays(ray_ids)`` forms the rays of global ray ids
(rows of ``RayGenerator``'s table: m H W + h W + w) on the device and is differentiable in ``xi``:

    cams = CameraRefinement.from_ray_generator(rg)
    pose_opt = torch.optim.Adam([cams.xi], 2e-3)
    rays, gt, ids = rg.select_batch("train", 4096)
    pose_opt.zero_grad()
    train_step(net, opt, cams.rays(ids), gt, N)        # back-propagates to its rays, so xi.grad is filled
    pose_opt.step()

``training.GraphedCameraTrainStep`` is the same joint step inside the captured graph.
"""
import torch

from .. import _lib


def _geometry(cam_params):
    H, W, f = int(cam_params[0]), int(cam_params[1]), float(cam_params[2])
    if H <= 0 or W <= 0 or not 0.0 < f < float("inf"):
        raise ValueError(f"cam_params must be [H, W, f] with H, W >= 1 and a finite f > 0, got {list(cam_params)!r}")
    return H, W, f


class _CameraRays(torch.autograd.Function):
    """nerf_amd_camera_rays; backward nerf_amd_camera_rays_backward (d loss / d xi, written per call: autograd accumulates)."""

    @staticmethod
    def forward(ctx, xi, cams, ids):
        ctx.cams, ctx.ids = cams, ids
        ctx.save_for_backward(xi)
        rays = torch.empty((ids.shape[0], 6), dtype=torch.float32, device=ids.device)
        cams._launch_rays(xi, ids, None, rays)
        return rays

    @staticmethod
    def backward(ctx, d_rays):
        (xi,) = ctx.saved_tensors
        g_xi = torch.empty_like(xi)
        ctx.cams._launch_backward(xi, ctx.ids, d_rays.float().contiguous(), g_xi)
        return g_xi, None, None


class CameraRefinement(torch.nn.Module):
    """``poses`` [M,4,4] or [M,3,4] (any device; kept on ``device`` as [M,3,4] fp32), ``cam_params`` = [H, W, f] shared by
    the M images.  ``xi`` [M,6] is the parameter, zeros at first: the rays then are ``generate_rays(poses[m])`` bit for bit."""

    def __init__(self, poses, cam_params, device="cuda"):
        super().__init__()
        self.H, self.W, self.f = _geometry(cam_params)
        p = torch.as_tensor(poses)
        if p.dim() != 3 or p.shape[0] < 1 or tuple(p.shape[1:]) not in ((4, 4), (3, 4)):
            raise RuntimeError(f"poses must be [M,4,4] or [M,3,4] with M >= 1, got {tuple(p.shape)}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"CameraRefinement lives on the GPU (got device {device}); this package has no CPU path")
        self.register_buffer("poses0", p[:, :3, :4].to(torch.float32).to(device).contiguous())
        self.xi = torch.nn.Parameter(torch.zeros((p.shape[0], 6), dtype=torch.float32, device=device))

    @classmethod
    def from_ray_generator(cls, rg, mode="train"):
        """The poses of ``rg.samples[mode][i]['transform']`` (RayGenerator.from_samples), on the device of its table."""
        import numpy as np
        if rg.samples is None or rg.cam_params is None or not rg.samples.get(mode):
            raise RuntimeError(f"the RayGenerator holds no poses for mode {mode!r} (build it with RayGenerator.from_samples)")
        poses = torch.from_numpy(np.stack([np.asarray(s["transform"], dtype=np.float32) for s in rg.samples[mode]]))
        cams = cls(poses, rg.cam_params, rg.rays_dataset[mode].device)
        if cams.n_rays != int(rg.rays_dataset[mode].shape[0]):
            raise RuntimeError(f"{cams.M} images of {cams.H} x {cams.W} are {cams.n_rays} rays, the table holds "
                               f"{int(rg.rays_dataset[mode].shape[0])}")
        return cams

    @property
    def M(self):
        return int(self.poses0.shape[0])

    @property
    def n_rays(self):
        """Length of the ray table these cameras span: M H W."""
        return self.M * self.H * self.W

    # ---- the three entry points --------------------------------------------------------------------------------------
    def _launch_rays(self, xi, ids, ids_copy, rays, stream=None):
        _lib.launch("nerf_amd_camera_rays", self.poses0, xi, ids, ids_copy, self.H, self.W, self.f, rays, int(ids.shape[0]),
                    self.M, dev=self.poses0.device, stream=stream)

    def _launch_backward(self, xi, ids, d_rays, g_xi, stream=None):
        _lib.launch("nerf_amd_camera_rays_backward", self.poses0, xi, ids, d_rays, self.H, self.W, self.f, g_xi, None,
                    int(ids.shape[0]), self.M, dev=self.poses0.device, stream=stream)

    def rays(self, ray_ids):
        """Rays [B,6] of the global ray ids [B] (int64, on the cameras' device), differentiable in ``xi``.  An id outside
        [0, M H W) gives a NaN row and no gradient."""
        if not torch.is_tensor(ray_ids) or ray_ids.dtype != torch.int64 or ray_ids.dim() != 1:
            raise RuntimeError("ray_ids must be a 1-d int64 tensor")
        if ray_ids.device != self.poses0.device:
            raise RuntimeError(f"ray_ids live on {ray_ids.device}, the cameras on {self.poses0.device}")
        return _CameraRays.apply(self.xi, self, ray_ids.contiguous())

    @torch.no_grad()
    def poses(self):
        """The corrected poses [M,4,4] (for ``render_view``): the bits the rays are formed from."""
        dev = self.poses0.device
        top = torch.empty((self.M, 3, 4), dtype=torch.float32, device=dev)
        _lib.launch("nerf_amd_camera_poses", self.poses0, self.xi, top, self.M, dev=dev)
        out = torch.zeros((self.M, 4, 4), dtype=torch.float32, device=dev)
        out[:, :3] = top
        out[:, 3, 3] = 1.0
        return out

    def pose(self, i):
        """The corrected pose [4,4] of image ``i``."""
        return self.poses()[int(i)]
