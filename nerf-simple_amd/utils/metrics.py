"""Image quality on the device: squared error, PSNR and SSIM of rendered views against ground truth (not in the reference,
whose only measure is ``img_psnr`` of train.py:21-26 on host tensors).

``image_metrics`` compares image pairs where they lie -- ``render_view``'s [H W, 4] pixels against the [H W, 3] rows of
``RayGenerator.colours`` -- through nerf_amd_image_metrics (csrc/image_metrics.hip; the definition is include/nerf_amd.h and,
in float64, tests/ssim_model.py) and returns device tensors without a host synchronisation.  ``evaluate`` is the validation
loop nobody should hand-write: for every view take the pose from ``rg.samples``, render through the chosen path, compare with
the slice of ``rg.colours`` that already sits in HBM; ONE read-back after the last view.

SSIM is tf.image.ssim(max_val=1) / skimage's structural_similarity(gaussian_weights=True, use_sample_covariance=False,
data_range=1): an 11 x 11 Gaussian window (sigma 1.5), no padding, the mean over positions and channels.  LPIPS needs network
weights and is out of scope.  There is no CPU path: a CPU tensor is refused."""
from typing import NamedTuple, Optional

import torch

from .. import _lib

SSIM_WINDOW = 11


class ImageMetrics(NamedTuple):
    """Per image, on the device, float64: ``mse`` [M], ``psnr`` [M] (peak 1), ``psnr_ref`` [M] (the reference's img_psnr: peak
    max(gt)), ``ssim`` [M] and ``ssim_rgb`` [M,3] (None without SSIM), ``sse`` [M,3], ``max_gt`` [M]; ``map`` [M, H-10, W-10, 3]
    fp32 on request."""
    mse: torch.Tensor
    psnr: torch.Tensor
    psnr_ref: torch.Tensor
    ssim: Optional[torch.Tensor]
    ssim_rgb: Optional[torch.Tensor]
    sse: torch.Tensor
    max_gt: torch.Tensor
    map: Optional[torch.Tensor] = None


def _check_images(pred, gt, H, W, ssim):
    """(M, C_pred, C_gt) of two image stacks [M*H*W, C], [M, H, W, C] or [H, W, C], C >= 3 -- or a RuntimeError, judged on
    the arguments alone: nothing is launched, drawn or copied before every refusal has had its turn (the device last)."""
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise RuntimeError(f"image_metrics: H and W must be positive, got {H} x {W}")
    counts = []
    for name, t in (("pred", pred), ("gt", gt)):
        if not torch.is_tensor(t):
            raise RuntimeError(f"image_metrics: {name} must be a torch tensor")
        if t.dtype != torch.float32:
            raise RuntimeError(f"image_metrics: {name} must be float32, got {t.dtype}")
        if t.dim() not in (2, 3, 4) or t.shape[-1] < 3:
            raise RuntimeError(f"image_metrics: {name} must be [M*H*W, C], [M, H, W, C] or [H, W, C] with at least 3 columns, "
                               f"got {tuple(t.shape)}")
        if t.dim() == 2:
            if t.shape[0] == 0 or t.shape[0] % (H * W):
                raise RuntimeError(f"image_metrics: {name} has {t.shape[0]} rows, not a positive multiple of H W = {H * W}")
            counts.append(t.shape[0] // (H * W))
        else:
            if tuple(t.shape[-3:-1]) != (H, W) or t.shape[0] == 0:
                raise RuntimeError(f"image_metrics: {name} must be [H, W, C] = [{H}, {W}, C] (or a stack of them), got {tuple(t.shape)}")
            counts.append(t.shape[0] if t.dim() == 4 else 1)
    if counts[0] != counts[1]:
        raise RuntimeError(f"image_metrics: pred holds {counts[0]} images of {H} x {W} and gt {counts[1]}: the shapes do not agree")
    if ssim and (H < SSIM_WINDOW or W < SSIM_WINDOW):
        raise RuntimeError(f"image_metrics: SSIM needs one 11 x 11 window, got {H} x {W} (NERF_AMD_EUNSUP; ssim=False for the "
                           "squared error alone)")
    _lib.require_cuda_f32(pred, "pred")
    _lib.require_cuda_f32(gt, "gt")
    if pred.device != gt.device:
        raise RuntimeError(f"image_metrics: pred is on {pred.device} and gt on {gt.device}")
    return counts[0], int(pred.shape[-1]), int(gt.shape[-1])


def _rows(t):
    """The tensor as rows read in place: (2-D view, row stride in floats).  Only a layout whose rows are not evenly spaced
    runs of floats is copied."""
    t2 = t.reshape(-1, t.shape[-1])
    if t2.stride(1) != 1 or (t2.shape[0] > 1 and t2.stride(0) < 3):
        t2 = t2.contiguous()
    return t2, (int(t2.stride(0)) if t2.shape[0] > 1 else int(t2.shape[1]))


def _workspace(M, H, W, dev):
    n = int(_lib.lib().nerf_amd_image_metrics_workspace_bytes(M, H, W))
    if n < 0:
        _lib.check(n, "nerf_amd_image_metrics_workspace_bytes")
    return torch.empty(max(n, 8), dtype=torch.uint8, device=dev)


def _launch(pred, gt, M, H, W, sums, ssim_rgb, ssim_map, workspace):
    p2, ps = _rows(pred)
    g2, gs = _rows(gt)
    _lib.launch("nerf_amd_image_metrics", p2, ps, g2, gs, sums, ssim_rgb, ssim_map, workspace, M, H, W, dev=p2.device)


def _derive(sums, ssim_rgb, H, W, ssim_map=None):
    """The reported quantities from the kernel's sums, in double, on the device."""
    sse, max_gt = sums[:, :3], sums[:, 3]
    mse = sse.sum(1) / (3 * H * W)
    psnr = -10.0 * torch.log10(mse)
    psnr_ref = 20.0 * torch.log10(max_gt) + psnr
    return ImageMetrics(mse, psnr, psnr_ref, None if ssim_rgb is None else ssim_rgb.sum(1) / 3.0, ssim_rgb, sse, max_gt, ssim_map)


def image_metrics(pred, gt, H, W, *, ssim=True, ssim_map=False):
    """``ImageMetrics`` of M image pairs.  pred, gt: [M*H*W, C], [M, H, W, C] or [H, W, C], fp32 on the GPU, C >= 3 -- columns
    beyond the third are never read (a view's disparity column), so the two may differ in C.  ``ssim=False``: squared error,
    PSNR and max(gt) only, for any H, W >= 1.  ``ssim_map=True`` also returns the per-position map.  Launches on the current
    stream and never synchronises with the host."""
    want_ssim = bool(ssim or ssim_map)
    M, _, _ = _check_images(pred, gt, H, W, want_ssim)
    H, W, dev = int(H), int(W), pred.device
    sums = torch.empty((M, 4), dtype=torch.float64, device=dev)
    rgb = torch.empty((M, 3), dtype=torch.float64, device=dev) if want_ssim else None
    smap = torch.empty((M, H - 10, W - 10, 3), dtype=torch.float32, device=dev) if ssim_map else None
    _launch(pred, gt, M, H, W, sums, rgb, smap, _workspace(M, H, W, dev))
    return _derive(sums, rgb, H, W, smap)


def ssim(pred, gt, H, W):
    """SSIM per image [M] (float64, on the device)."""
    return image_metrics(pred, gt, H, W).ssim


def psnr(pred, gt):
    """-10 log10(mse) per image, peak 1 (float64, on the device) of [H, W, C] images, a stack [M, H, W, C], or two tables of
    rows [n, C] taken as one image."""
    if torch.is_tensor(pred) and pred.dim() == 2:
        return image_metrics(pred, gt, 1, pred.shape[0], ssim=False).psnr
    return image_metrics(pred, gt, pred.shape[-3], pred.shape[-2], ssim=False).psnr


def _evaluate(render, poses, gt_of, H, W, ssim, dev):
    V, HW = len(poses), H * W
    sums = torch.empty((V, 4), dtype=torch.float64, device=dev)
    rgb = torch.empty((V, 3), dtype=torch.float64, device=dev) if ssim else None
    ws = _workspace(1, H, W, dev)
    with torch.no_grad():
        for v, pose in enumerate(poses):
            pixels, gt = render(pose), gt_of(v)
            _check_images(pixels, gt, H, W, ssim)
            if pixels.dim() != 2 or pixels.shape[0] != HW:
                raise RuntimeError(f"evaluate_views: render(pose) must return pixels [H W, >= 3] = [{HW}, C], got {tuple(pixels.shape)}")
            _launch(pixels, gt, 1, H, W, sums[v:v + 1], None if rgb is None else rgb[v:v + 1], None, ws)
    m = _derive(sums, rgb, H, W)
    cols = [m.mse, m.psnr, m.psnr_ref] + ([m.ssim, m.ssim_rgb[:, 0], m.ssim_rgb[:, 1], m.ssim_rgb[:, 2]] if ssim else [])
    host = torch.stack(cols, 1).cpu() if V else torch.empty((0, len(cols)), dtype=torch.float64)      # the ONE read-back
    out = {"views": V, "mse": host[:, 0].tolist(), "psnr": host[:, 1].tolist(), "psnr_ref": host[:, 2].tolist()}
    if ssim:
        out["ssim"] = host[:, 3].tolist()
        out["ssim_rgb"] = host[:, 4:7].tolist()
    out["mean"] = {k: (sum(out[k]) / V if V else float("nan")) for k in ("mse", "psnr", "psnr_ref", "ssim") if k in out}
    return out


def evaluate_views(render, poses, gt, H, W, *, ssim=True):
    """Metrics of ``render(pose)`` -- pixels [H W, >= 3] on the device -- for every pose against ``gt`` [len(poses) H W, 3] on
    the device.  The renders run under ``torch.no_grad()``; every view's sums land in preallocated rows and come back in one
    copy after the last view.  Returns {'views', 'mse', 'psnr', 'psnr_ref', 'ssim', 'ssim_rgb'} as per-view lists and 'mean',
    their means over the views ('psnr': peak 1; 'psnr_ref': the reference's img_psnr, peak max(gt))."""
    H, W, V = int(H), int(W), len(poses)
    if V == 0:
        raise RuntimeError("evaluate_views: no poses")
    if not torch.is_tensor(gt) or gt.dim() != 2 or gt.shape[0] != V * H * W:
        raise RuntimeError(f"evaluate_views: gt must be [len(poses) H W, 3] = [{V * H * W}, 3], got "
                           f"{tuple(gt.shape) if torch.is_tensor(gt) else type(gt).__name__}")
    _check_images(gt, gt, H, W, ssim)
    return _evaluate(render, list(poses), lambda v: gt[v * H * W:(v + 1) * H * W], H, W, bool(ssim), gt.device)


def evaluate(net, rg, im_set='val', idxs=None, *, N=128, render=None, ssim=True, **render_kw):
    """Metrics of a trained model over the views of ``rg.samples[im_set]`` (all of them, or ``idxs``): the pose of view i is
    ``rg.samples[im_set][i]['transform']``, its ground truth the rows ``rg.colours[im_set][i H W:(i+1) H W]``, which are
    resident and are not copied.  The default render is ``render_view(net, pose, rg.cam_params, N=N, **render_kw)``, so
    ``occupancy=``, ``terminate=``, ``background=``, ``box=``, ``device_rng=``, ``precision=`` pass through; ``render=`` -- a function
    pose -> pixels [H W, >= 3] -- takes the other paths, e.g.
    ``lambda pose: render_guided_view(net, pose, rg.cam_params, 64, 128, prop, occupancy=occ)``.  Returns what
    ``evaluate_views`` returns, plus 'idxs'."""
    if getattr(rg, "samples", None) is None or getattr(rg, "cam_params", None) is None:
        raise RuntimeError("evaluate: this RayGenerator carries no samples / cam_params (it was built by from_tables): the poses "
                           "are not known to it -- use evaluate_views(render, poses, gt, H, W)")
    if render is not None and render_kw:
        raise RuntimeError(f"evaluate: render= is given, so {sorted(render_kw)} would go nowhere: bind them in the render function")
    if im_set not in rg.samples or im_set not in rg.colours:
        raise RuntimeError(f"evaluate: no views / colour table for im_set {im_set!r}")
    items, table = rg.samples[im_set], rg.colours[im_set]
    H, W = int(rg.cam_params[0]), int(rg.cam_params[1])
    idxs = list(range(len(items))) if idxs is None else [int(i) for i in idxs]
    if not idxs or min(idxs) < 0 or max(idxs) >= len(items):
        raise RuntimeError(f"evaluate: idxs must name views 0..{len(items) - 1} of {im_set!r}, got {idxs}")
    _check_images(table, table, H, W, ssim)
    if render is None:
        from .rendering import render_view
        cam = rg.cam_params

        def render(pose):
            return render_view(net, pose, cam, N=N, **render_kw)
    import numpy as np
    poses = [np.asarray(items[i]["transform"], dtype=np.float32) for i in idxs]
    out = _evaluate(render, poses, lambda v: table[idxs[v] * H * W:(idxs[v] + 1) * H * W], H, W, bool(ssim), table.device)
    out["idxs"] = idxs
    return out
