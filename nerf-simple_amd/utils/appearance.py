"""Appearance: one learnable colour correction per training image, trained beside the network (not in the reference, whose
frames share one exposure; Urban Radiance Fields learns an affine map per image, instant-ngp and nerfstudio a per-image
exposure).  Validation and novel views are rendered uncorrected -- ``evaluate`` does not know this module, which is the point.

Image m of M holds ``theta[m] = (a[3], b[3])``, zeros at first; a ray of it is compared with its pixel behind

    c' = (1 + a) * c + b            c = the compositor's rgb, before any clip

(csrc/appearance_device.h: three separately rounded fp32 operations per channel).  The image of a ray
is ``ray_id // HW`` of its global ray id, the row of ``RayGenerator``'s table:

    app = AppearanceCorrection.from_ray_generator(rg)
    app_opt = torch.optim.Adam([app.theta], 1e-3)
    rays, gt, ids = rg.select_batch("train", 4096)
    rgb = render_nerf(rays, net, N, ...)[0]
    loss = training.mse_loss(app(rgb, ids), gt)
    loss.backward()                                    # fills app.theta.grad beside the network's gradients

``training.GraphedAppearanceTrainStep`` is the same joint step inside the captured graph.  The gains and the network's colour
scale share a gauge; ``reg`` (a ridge on theta) and ``frozen`` (images held at the identity) fix it.  Out of scope: the
masked, hierarchical, guided and camera steppers, a full 3x3 colour matrix, exponential gains, a correction at evaluation time.
"""
import torch

from .. import _lib


class _Appearance(torch.autograd.Function):
    """gather + apply; backward apply_backward + reduce (d loss / d theta written per call: autograd accumulates)."""

    @staticmethod
    def forward(ctx, rgb, theta, app, ids):
        B, dev = int(ids.shape[0]), theta.device
        theta_ray = torch.empty((B, 6), dtype=torch.float32, device=dev)
        out = torch.empty((B, 3), dtype=torch.float32, device=dev)
        if B:
            _lib.launch("nerf_amd_appearance_gather", theta, ids, None, app.HW, theta_ray, B, app.M, dev=dev)
            _lib.launch("nerf_amd_appearance_apply", rgb, theta_ray, 6, out, B, dev=dev)
        ctx.app, ctx.ids = app, ids
        ctx.save_for_backward(rgb, theta, theta_ray)
        return out

    @staticmethod
    def backward(ctx, g_out):
        rgb, theta, theta_ray = ctx.saved_tensors
        app, ids = ctx.app, ctx.ids
        B = int(ids.shape[0])
        g_out = g_out.float().contiguous()
        g_rgb, g_ray = torch.empty_like(rgb), torch.empty_like(theta_ray)
        g_theta = torch.zeros_like(theta)
        if B:
            _lib.launch("nerf_amd_appearance_apply_backward", g_out, rgb, theta_ray, 6, g_rgb, g_ray, B, dev=theta.device)
            _lib.launch("nerf_amd_appearance_reduce", g_ray, ids, app.HW, theta, app.reg, app._frozen_arg, g_theta, B, app.M,
                        dev=theta.device)
        return g_rgb, g_theta, None, None


class AppearanceCorrection(torch.nn.Module):
    """``M`` images of ``HW`` pixels each.  ``theta`` [M,6] fp32 is the parameter (``state_dict`` carries it).  ``reg``: the
    weight of the ridge (reg / 2) sum ||theta||^2, whose gradient ``reg * theta`` reaches every image at every backward, with
    or without a ray of it in the batch (the loss value stays the MSE).  ``frozen``: indices of images whose gradient is
    exactly zero (no ridge either): an image held at the identity anchors the colour scale."""

    def __init__(self, M, HW, device="cuda", reg=0.0, frozen=()):
        super().__init__()
        M, HW, reg = int(M), int(HW), float(reg)
        if M < 1 or HW < 1:
            raise RuntimeError(f"AppearanceCorrection needs M >= 1 images of HW >= 1 pixels, got M = {M}, HW = {HW}")
        if not 0.0 <= reg < float("inf"):
            raise RuntimeError(f"reg must be finite and >= 0, got {reg}")
        frozen = sorted({int(i) for i in frozen})
        if frozen and (frozen[0] < 0 or frozen[-1] >= M):
            raise RuntimeError(f"frozen holds an image outside [0, {M}): {frozen}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"AppearanceCorrection lives on the GPU (got device {device}); this package has no CPU path")
        self.M, self.HW, self.reg, self.frozen = M, HW, reg, tuple(frozen)
        self.theta = torch.nn.Parameter(torch.zeros((M, 6), dtype=torch.float32, device=device))
        mask = torch.zeros(M, dtype=torch.int32)
        mask[list(frozen)] = 1
        self.register_buffer("frozen_mask", mask.to(device), persistent=False)

    @classmethod
    def from_ray_generator(cls, rg, mode="train", **kw):
        """One row per image of ``rg``'s table for ``mode`` (a ``RayGenerator`` that knows its image size), on its device."""
        if rg.cam_params is None:
            raise RuntimeError("the RayGenerator does not know its image size (build it with RayGenerator.from_samples)")
        table = rg.rays_dataset[mode]
        HW, n = int(rg.cam_params[0]) * int(rg.cam_params[1]), int(table.shape[0])
        if HW < 1 or n % HW:
            raise RuntimeError(f"a table of {n} rays is not a whole number of images of {HW} pixels")
        return cls(n // HW, HW, table.device, **kw)

    @property
    def n_rays(self):
        """Length of the ray table this correction spans: M HW."""
        return self.M * self.HW

    @property
    def _frozen_arg(self):
        return self.frozen_mask if self.frozen else None

    def forward(self, rgb, ray_ids):
        """c' [B,3] of the colours ``rgb`` [B,3] of the rays with global ids ``ray_ids`` [B] (int64), differentiable in ``rgb``
        and in ``theta``.  An id outside [0, M HW) gives a NaN colour and no gradient to any image."""
        dev = self.theta.device
        _lib.require_cuda_f32(rgb, "rgb")
        if not torch.is_tensor(ray_ids) or ray_ids.dtype != torch.int64 or ray_ids.dim() != 1:
            raise RuntimeError("ray_ids must be a 1-d int64 tensor")
        if rgb.dim() != 2 or tuple(rgb.shape) != (int(ray_ids.shape[0]), 3):
            raise RuntimeError(f"rgb must be [{int(ray_ids.shape[0])},3] (one colour per ray id), got {tuple(rgb.shape)}")
        if rgb.device != dev or ray_ids.device != dev:
            raise RuntimeError(f"rgb lives on {rgb.device}, ray_ids on {ray_ids.device}, the correction on {dev}")
        return _Appearance.apply(rgb.contiguous(), self.theta, self, ray_ids.contiguous())

    @torch.no_grad()
    def gains(self):
        """[M,3]: fl(1 + a), the factor every colour of image m is multiplied by."""
        return 1 + self.theta[:, :3]

    @torch.no_grad()
    def bias(self):
        """[M,3]: b."""
        return self.theta[:, 3:].clone()
