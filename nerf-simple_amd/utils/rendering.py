"""Drop-in for the hot path of the reference's utils/rendering.py.

``render_nerf`` (alias ``render_rays``) and ``volume_render`` keep the
reference's names, positional arguments, defaults and return order
(reference utils/rendering.py:13,47); the bodies are HIP kernels behind
libnerf_amd.so.  ``render_image`` / ``render_poses`` reproduce the batching and
clipping semantics of the reference's image drivers (utils/rendering.py:88-153)
without the video writer.

Jitter: in parity mode (default) ``render_nerf`` draws exactly one
``torch.rand(B, N)`` from the CPU default generator per call, as the reference
does (utils/rendering.py:28), so a seeded run consumes the RNG identically.
``u=`` / ``ts=`` inject explicit jitter / sample positions; ``device_rng=True``
draws jitter from a counter RNG on the GPU instead (no PCIe copy, results
independent of batching and sharding, not bit-comparable to the reference).

Gradients: ``render_nerf`` is differentiable in its rays, as the reference is: with ``rays.requires_grad`` (and
grad enabled) ``d loss / d rays`` comes back through autograd for a trainable or a frozen ``Nerf`` and for any
foreign net whose forward is differentiable in its input (camera-pose refinement, pose estimation against a
trained NeRF: INTEGRATION.md).  The sample positions carry no gradient (jitter, ``u=`` and ``ts=`` are constants),
and a direct ``volume_render`` call gives none to ``ts`` / ``dirs``.  Precision under autograd is the training
path's: 'fp16' / 'bf16' modules run the bf16 training kernels, 'fp32' modules exact fp32.
"""
import torch
from tqdm import tqdm

from .. import _lib
from . import box as box_mod, controls as controls_mod, jitter
from .controls import background_arg as _background_arg      # the name tests/test_background_cpu.py holds the shape rule by
from .host_rng import ReferenceJitter
from .jitter import tbins as _tbins
from .nets import Nerf, guarded_launch

ALL_OUTPUTS = ("rgb", "disp", "alpha", "acc", "w")
_FUSED_MAX_N = 768          # csrc/nerf_layout.h FUSED_RENDER_MAX_N: rays the one-launch render composites in its LDS ring


def _per_sample(t_, N):
    """alpha / w as the reference shapes them: [B,N], except [B,0] at N == 1, where its delta construction
    leaves the sample axis empty (utils/rendering.py:60-61; the kernels reproduce rgb = acc = 0, disparity = NaN)."""
    return t_ if (t_ is None or N != 1) else t_[:, :0]


def _five_outputs(B, N, outputs, dev):
    """Uninitialised buffers for (rgb [B,3], disp [B], alpha [B,N], acc [B], w [B,N]); alpha / w only when
    `outputs` names them, else None (the kernels skip a NULL output)."""
    def buf(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)
    rgb, disp, acc = buf(B, 3), buf(B), buf(B)
    return rgb, disp, buf(B, N) if "alpha" in outputs else None, acc, buf(B, N) if "w" in outputs else None


def volume_render(nerf_outs, ts, dirs, *, outputs=ALL_OUTPUTS, background=None):
    """nerf_outs [B,N,4], ts [B,N], dirs [B,3] -> (rgb [B,3], disp [B], alpha [B,N],
    acc [B], w [B,N])  (reference utils/rendering.py:47-85).  The second output is
    disparity; acc == 0 yields NaN there, as in the reference.
    background: a colour [3] or one per ray [B,3] behind the volume -- rgb becomes rgb + (1 - acc) background (fp32, each
    operation rounded on its own); the other four outputs are what they were."""
    _lib.require_cuda_f32(nerf_outs, "nerf_outs")
    _lib.require_cuda_f32(ts, "ts")
    _lib.require_cuda_f32(dirs, "dirs")
    if nerf_outs.dim() != 3 or nerf_outs.shape[-1] != 4:
        raise RuntimeError("nerf_outs must be [B, N, 4]")
    B, N = nerf_outs.shape[0], nerf_outs.shape[1]
    if tuple(ts.shape) != (B, N) or tuple(dirs.shape) != (B, 3):
        raise RuntimeError("ts must be [B, N] and dirs [B, 3]")
    c = None if background is None else controls_mod.resolve(controls_mod.Controls(background), B, nerf_outs.device)
    if torch.is_grad_enabled() and nerf_outs.requires_grad:
        from ..training import volume_render_autograd
        out = volume_render_autograd(nerf_outs, ts, dirs)
        return out if c is None else (controls_mod.Background.apply(out[0], out[3], c.bg, c.stride),) + tuple(out[1:])
    dev = nerf_outs.device
    raw, ts, dirs = nerf_outs.detach().contiguous(), ts.detach().contiguous(), dirs.detach().contiguous()
    rgb, disp, alpha, acc, w = _five_outputs(B, N, outputs, dev)
    _lib.launch("nerf_amd_volume_render", raw, ts, dirs, 3, rgb, disp, alpha, acc, w, B, N, dev=dev)
    out = rgb, disp, _per_sample(alpha, N), acc, _per_sample(w, N)
    return controls_mod.blended(out, c)


def render_nerf(rays, net, N, tn=2, tf=6, *, u=None, ts=None, outputs=ALL_OUTPUTS,
                precision=None, device_rng=False, seed=0, ray_id0=0, occupancy=None, terminate=None,
                background=None, sigma_noise=0.0, noise_seed=0, controls=None, box=None):
    """Stratified sampling along rays, NeRF query, compositing
    (reference utils/rendering.py:13-45).

    rays [B,6] = [origin, direction] on the GPU; net: a ``Nerf`` (fused HIP path)
    or any object with ``.forward(query_pts[P,6]) -> [P,4]`` (generic path: the
    net runs as given, sampling and compositing still run here).
    Returns (rgb [B,3], disp [B], alpha [B,N], acc [B], w [B,N]); alpha / w are
    None when left out of ``outputs``.

    occupancy: an ``OccupancyGrid`` (utils/occupancy.py) -- the network is evaluated at the live samples only and a dead
    sample contributes exactly nothing (the masked render; one host synchronisation per call).  Inference only: a
    grad-enabled call on a trainable net or on rays that require grad raises RuntimeError (call it under
    ``torch.no_grad()``), and so do other network sizes and foreign nets -- nothing falls back to the dense render.

    terminate: an ``EarlyTermination(eps, slab)`` (utils/occupancy.py) -- early ray termination: the samples are evaluated
    slab by slab and a ray whose transmittance has fallen below eps evaluates nothing more (the masked render under the
    evaluated mask; at most ceil(N / slab) + 1 host synchronisations).  With ``occupancy`` it runs on that grid, without one on
    an all-live grid; the masked render's conditions hold either way.

    background: a colour [3] (or one per ray [B,3]) behind the volume: rgb becomes rgb + (1 - acc) background, fp32 with
    every operation rounded on its own; disp, alpha, acc and w are what they were, and the background carries no gradient.
    sigma_noise: standard deviation of Gaussian noise added to the raw density in front of the softplus (the reference's
    open ``## TODO add gaussian noise regularizer``, utils/rendering.py:63) -- a REGULARISER: a call that does not train
    (no_grad, a frozen net and rays without grad) raises RuntimeError.  The noise comes from the counter RNG keyed by
    ``noise_seed`` and the global sample id (``ray_id0``), whatever the jitter source; pass a new ``noise_seed`` per step.
    Both serve the dense path only: with ``occupancy`` or ``terminate`` they raise RuntimeError before anything is drawn
    or launched.

    controls: a ``training.Controls`` -- without a grid the equivalent of the three keywords above (both given: ValueError);
    with ``occupancy`` the background behind the masked render: rgb becomes rgb + (1 - acc) background through the same blend,
    the other four outputs are what they were.  ``controls.sigma_noise > 0`` behind a grid raises the regulariser's
    RuntimeError, a non-zero ``controls.distortion`` ValueError, ``terminate=`` with it RuntimeError.

    box: a ``SceneBox`` or a ``GridSpan`` (utils/box.py; DESIGN.md sections 33 and 39) -- each ray's N samples are placed inside the box instead of in
    [tn, tf] (a ray that misses keeps [tn, tf]): ``box.positions(rays, N, tn, tf, u=, device_rng=, seed=, ray_id0=)`` is formed
    once, where the jitter would be drawn, and the call goes on as its ``ts=`` path -- so it composes with everything that
    path serves (``occupancy``, ``terminate``, the controls, every precision, foreign nets).  The positions are constants:
    no gradient, and d loss / d rays ignores the dependence of the interval on the ray (the fine sampler's rule).
    ``box=`` together with ``ts=`` is a ValueError.
    """
    box_mod.check_box(box, ts=ts)
    c = controls_mod.from_keywords(controls, {"occupancy": occupancy, "terminate": terminate}, background=background,
                                   sigma_noise=sigma_noise, noise_seed=noise_seed)
    if controls is not None:
        controls_mod.render_only(c, terminate, " (train_step(..., controls=))")
        if occupancy is not None and c.sigma_noise > 0:
            controls_mod.refuse_noise("the masked inference render trains nothing")
    if c is not None:
        c = controls_mod.resolve(c, _lib.require_rays(rays), rays.device, ray_id0)
    return _render_nerf(rays, net, N, tn, tf, c, u=u, ts=ts, outputs=outputs, precision=precision, device_rng=device_rng, seed=seed,
                        ray_id0=ray_id0, occupancy=occupancy, terminate=terminate, box=box)


render_rays = render_nerf      # the name BASELINE.json uses for the same function


def _render_nerf(rays, net, N, tn, tf, c, *, u=None, ts=None, outputs=ALL_OUTPUTS, precision=None, device_rng=False, seed=0,
                 ray_id0=0, occupancy=None, terminate=None, box=None):
    """The body of ``render_nerf`` behind its controls preamble.  ``c``: the ``Resolved`` controls or None -- without a grid the
    background and / or the noise; with ``occupancy`` the background behind the masked render."""
    B, N = _lib.require_rays(rays), int(N)
    dev = rays.device
    # d loss / d rays (utils/rendering.py:31-40 is differentiable in the rays): autograd runs even for a frozen net
    rays_grad = torch.is_grad_enabled() and rays.requires_grad
    rays_in = rays.contiguous() if rays_grad else None
    rays = rays.detach().contiguous()

    fused = isinstance(net, Nerf) and net._fused_ok()
    training = fused and torch.is_grad_enabled() and (rays_grad or any(p.requires_grad for p in net.parameters()))
    if c is not None and c.std > 0:
        trains = training or (not fused and torch.is_grad_enabled() and (
            rays_grad or any(p.requires_grad for p in getattr(net, "parameters", lambda: ())())))
        if not trains:
            controls_mod.refuse_noise("this call trains nothing (no_grad, or no parameter and no ray requires grad)")
    if terminate is not None:
        from .occupancy import check_terminable
        check_terminable(terminate, occupancy, net, rays_grad)
    elif occupancy is not None:
        from .occupancy import check_renderable
        check_renderable(occupancy, net, rays_grad)
    # everything that can raise cheaply is checked BEFORE the jitter is drawn, so a failed call
    # leaves torch's CPU generator untouched
    jitter.check(B, N, u=u, ts=ts)
    if box is not None:
        box_mod.check_interval(N, tn, tf)
    code = None
    if fused and not training:
        code = _lib.precision_of(net, precision)
        net.packed_weights(code)              # packs now if it has to: errors surface before the jitter is drawn
    if box is not None:                       # the box's positions, then the ts= path
        jit, flags, pending_rng = box_mod.single(box, rays, N, tn, tf, u=u, device_rng=device_rng, seed=seed, ray_id0=ray_id0)
    else:
        jit, flags, pending_rng = jitter.single(B, N, dev, u=u, ts=ts, device_rng=device_rng)
    # the reference's |x| > 1 warning (utils/xyz.py:8-9, raised inside net.forward's positional_encoder): verdict formed on
    # the device from the first / last sample of every ray, raised lazily (xyz.range_check_rays); a foreign net encodes
    # its own inputs and warns (or not) by itself
    if fused:
        from .xyz import range_check_rays
        tb = jitter.tbins(tn, tf, N, dev, flags)
        range_check_rays(rays, jit, tb, flags, seed, ray_id0, N)
    if pending_rng is not None and not fused:
        pending_rng.finish()                  # the net's own forward follows: the generator must be current
        pending_rng = None
    if terminate is not None or occupancy is not None:
        from .occupancy import render_masked, render_terminated
        try:
            if terminate is not None:
                return render_terminated(terminate, occupancy, rays, net, N, tb, jit, flags, seed, ray_id0, code, outputs)
            out = render_masked(occupancy, rays, net, N, tb, jit, flags, seed, ray_id0, code, outputs)
            return controls_mod.blended(out, c)
        finally:
            if pending_rng is not None:
                pending_rng.finish()
    if training:
        from ..training import render_nerf_autograd
        try:
            return render_nerf_autograd(rays_in if rays_grad else rays, net, N, tn, tf, jit, flags,
                                        net.precision if precision is None else precision,
                                        seed, ray_id0, c)
        finally:
            if pending_rng is not None:
                pending_rng.finish()          # the forward is enqueued behind the generator kernel: only that is awaited
    if not fused:
        return _render_generic(rays_in if rays_grad else rays, net, N, tn, tf, jit, flags, outputs, seed, ray_id0, c)

    def launch(code, packed):
        rgb, disp, alpha, acc, w = _render_forward(rays, jit, _tbins(tn, tf, N, dev), packed[0], code, flags, seed, ray_id0, N,
                                                   outputs)
        out = rgb, disp, _per_sample(alpha, N), acc, _per_sample(w, N)
        # with a background: the same one-launch render, then the blend (acc is always among the outputs)
        return controls_mod.blended(out, c)

    try:
        return guarded_launch([net], code, launch)     # fp16: range guard (nets.guarded_launch)
    finally:
        if pending_rng is not None:
            pending_rng.finish()              # the render is enqueued behind it: only the generator kernel is awaited


def _render_forward(rays, jit, tbins, image, code, flags, seed, ray_id0, N, outputs):
    """nerf_amd_render_forward with its outputs and its workspace: the five buffers of ``_five_outputs``, as the kernel left
    them (``render_nerf`` and ``render_view(background=)`` differ in the outputs they ask for and in the blend behind)."""
    B, dev = rays.size(0), rays.device
    out = _five_outputs(B, N, outputs, dev)
    ws = _lib.workspace(_lib.lib().nerf_amd_render_workspace_bytes(code, B, N), dev, floor=0)     # 0 bytes: the one-launch render
    _lib.launch("nerf_amd_render_forward", rays, jit, tbins, image, code, flags, int(seed), int(ray_id0), *out, ws, B, N,
                dev=dev)
    return out


def _render_generic(rays, net, N, tn, tf, jit, flags, outputs, seed, ray_id0, c=None):
    """Any other net object: sampling and query-point assembly in one HIP kernel (nerf_amd_query_points =
    utils/rendering.py:24-40; the same jitter sources as the fused path, counter RNG included), the net's own
    forward exactly as the reference calls it (:41), compositing by the HIP kernel with the directions taken
    from the rays (:37,43).  Gradients flow to whatever ``net.forward`` attaches to its output, and to the rays
    when they require grad (nerf_amd_query_points_backward)."""
    B, dev = rays.size(0), rays.device
    if torch.is_grad_enabled() and rays.requires_grad:
        q, ts = _QueryPoints.apply(rays, jit, _tbins(tn, tf, N, dev), flags, seed, ray_id0, N)
        rays = rays.detach()
    else:
        q, ts = _query_points(rays, jit, _tbins(tn, tf, N, dev), flags, seed, ray_id0, N)
    out = net.forward(q).reshape(B, N, 4).float()
    if torch.is_grad_enabled() and out.requires_grad:
        from ..training import composite_with_controls
        return composite_with_controls(out, ts, rays, True, c)
    if c is not None and c.std > 0:
        raise RuntimeError("sigma_noise is a training regulariser: the net's output carries no gradient")
    out = out.detach().contiguous()
    rgb, disp, alpha, acc, w = _five_outputs(B, N, outputs, dev)
    _lib.launch("nerf_amd_volume_render_rays", out, ts, rays, rgb, disp, alpha, acc, w, B, N, dev=dev)
    out = rgb, disp, _per_sample(alpha, N), acc, _per_sample(w, N)
    return controls_mod.blended(out, c)


def _query_points(rays, jit, tbins, flags, seed, ray_id0, N):
    """query points [B*N,6] and sample positions [B,N] of nerf_amd_query_points (utils/rendering.py:24-40)."""
    B, dev = rays.size(0), rays.device
    q = torch.empty((B * N, 6), dtype=torch.float32, device=dev)
    ts = torch.empty((B, N), dtype=torch.float32, device=dev)
    _lib.launch("nerf_amd_query_points", rays, jit, tbins, flags, int(seed), int(ray_id0), q, ts, B, N, dev=dev)
    return q, ts


class _QueryPoints(torch.autograd.Function):
    """rays [B,6] -> (query points [B*N,6], ts [B,N]) with the gradient to the rays: d_o = sum_n dx_n,
    d_d = sum_n t_n dx_n + (g - d_hat (d_hat . g)) / |d| (nerf_amd_query_points_backward)."""

    @staticmethod
    def forward(ctx, rays, jit, tbins, flags, seed, ray_id0, N):
        q, ts = _query_points(rays.detach(), jit, tbins, flags, seed, ray_id0, N)
        ctx.save_for_backward(rays, ts)
        ctx.N = N
        ctx.mark_non_differentiable(ts)
        return q, ts

    @staticmethod
    def backward(ctx, g_q, _g_ts):
        rays, ts = ctx.saved_tensors
        B, dev = rays.size(0), rays.device
        d_rays = torch.empty((B, 6), dtype=torch.float32, device=dev)
        g_q = g_q.contiguous().float()
        _lib.launch("nerf_amd_query_points_backward", rays, ts, g_q, d_rays, B, ctx.N, dev=dev)
        return d_rays, None, None, None, None, None, None


def _render_batched(rays, net, batch_size, N, tn, tf, u, progress, id_base=0, **kw):
    """Shared body of the image drivers (reference utils/rendering.py:98-108,
    139-151): per batch render_nerf under no_grad, clip rgb to [0,1] AFTER
    compositing, disparity un-clipped.  Unlike the reference's
    ``range(n // batch_size)`` the tail batch is rendered too."""
    n = rays.size(0)
    rgb = torch.empty((n, 3), dtype=torch.float32, device=rays.device)
    disp = torch.empty((n,), dtype=torch.float32, device=rays.device)
    background = kw.pop("background", None)          # one colour, or one per ray of this table: its rows follow the batches
    per_ray = torch.is_tensor(background) and background.dim() == 2
    if per_ray and background.shape[0] != n:
        raise controls_mod.background_shape(n, background.shape)
    if isinstance(net, Nerf) and net._fused_ok() and rays.is_cuda and 0 < n and N <= _FUSED_MAX_N:
        # The reference's batch_size bounds the [batch, N, ...] tensors of its per-sample path.  The fused render keeps
        # nothing per sample in HBM and its pixels do not depend on how the rays are batched (jitter rows follow the rays;
        # bit for bit: tests/test_gpu_parity.py test_headline_workload_properties), so the image is ONE launch: 40 launches
        # of 16,000 rays each end in a partly filled wave of tiles (+1.6 % at 800 x 800).  Longer rays (two-launch path,
        # 20 B per sample of workspace) and foreign nets keep the caller's batches.
        batch_size = n
    starts = range(0, n, batch_size)
    # The reference draws each batch's jitter inside render_nerf from the CPU generator: consecutive
    # pieces of one stream.  For the fused path they are all enqueued now on a side stream, so
    # batch k+1 is drawn while batch k renders (host_rng.ReferenceJitter); a generic ``net`` keeps
    # the per-call draw, since its forward may use the generator itself.
    ahead = None
    if (u is None and not kw.get("device_rng") and n > 0 and rays.is_cuda
            and isinstance(net, Nerf) and net._fused_ok()):
        ahead = ReferenceJitter([min(s + batch_size, n) - s for s in starts], N, rays.device)
    try:
        with torch.no_grad():
            for k, s in enumerate(tqdm(starts) if progress else starts):
                e = min(s + batch_size, n)
                uk = ahead.batch(k) if ahead is not None else (None if u is None else u[s:e])
                if background is not None:
                    kw["background"] = background[s:e] if per_ray else background
                r, d, _, _, _ = render_nerf(rays[s:e], net, N, tn, tf, u=uk,
                                            outputs=("rgb", "disp", "acc"), ray_id0=id_base + s, **kw)
                rgb[s:e] = torch.clip(r, 0., 1.)
                disp[s:e] = d
    finally:
        if ahead is not None:
            ahead.finish()
    return rgb, disp


def render_image(net, rg, batch_size=64000, im_idx=0, im_set='val', *, N=128, tn=2, tf=6,
                 u=None, progress=False, **kw):
    """Render image ``im_idx`` of ``rg``'s ``im_set`` (reference utils/rendering.py:88-113).
    ``rg`` is any object with the reference RayGenerator's fields
    ``samples[im_set][i]['img']`` and ``rays_dataset[im_set]`` ([n_img*H*W, 6]).
    Returns (rgb [1,H,W,3], disparity [1,H,W,1], gt [1,H,W,3]) on the CPU."""
    gt = rg.samples[im_set][im_idx]['img']
    H, W = gt.shape[0], gt.shape[1]
    dev = next(net.parameters()).device
    rays = rg.rays_dataset[im_set][im_idx * H * W:(im_idx + 1) * H * W, :].to(dev).float()
    rgb, disp = _render_batched(rays, net, batch_size, N, tn, tf, u, progress, **kw)
    return rgb.cpu().reshape(1, H, W, 3), disp.cpu().reshape(1, H, W, 1), gt.reshape(1, H, W, 3)


def render_poses(net, poses, cam_params, batch_size, savepath='', *, N=128, tn=2, tf=6,
                 u=None, progress=False, **kw):
    """Render one image per pose (reference utils/rendering.py:116-153).
    poses: list of [4,4] float tensors; cam_params [H,W,f].  Returns
    (rgb_imgs, disp_imgs): lists of numpy [H,W,3] / [H,W].  The reference's mp4
    writer (cv2, :155-160) is out of scope; ``savepath`` is accepted and ignored.

    The reference builds the ray table of every pose on the CPU (:129-134) and moves it to the GPU batch
    by batch; at 800x800 that table takes 0.2 s per pose on 8 cores -- three times the render -- and
    24 B per ray of PCIe.  Here each pose's rays come from the device generator (generate_rays, N1:
    the same table to the fma rounding of the 3-term rotation, 2.4e-7 absolute)."""
    H, W = cam_params[0], cam_params[1]
    dev = next(net.parameters()).device
    # The reference reads every image back as soon as it is rendered (:150-151, a blocking copy).  Here the copy of
    # pose i runs on a side stream into pinned memory while pose i+1 renders; the arrays are handed out after the last
    # copy has landed (the returned numpy arrays view that pinned memory).
    copier = torch.cuda.Stream(device=dev)
    rgb_host, disp_host = [], []
    for i in range(len(poses)):
        pose = poses[i].detach().cpu() if torch.is_tensor(poses[i]) else poses[i]
        rays = generate_rays(pose, cam_params, dev)
        ui = None if u is None else u[i * H * W:(i + 1) * H * W]
        rgb, disp = _render_batched(rays, net, batch_size, N, tn, tf, ui, progress,
                                    id_base=i * H * W, **kw)
        rgb_h = torch.empty((H, W, 3), dtype=torch.float32).pin_memory()
        disp_h = torch.empty((H, W), dtype=torch.float32).pin_memory()
        copier.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(copier):
            rgb_h.copy_(rgb.view(H, W, 3), non_blocking=True)
            disp_h.copy_(disp.view(H, W), non_blocking=True)
        rgb.record_stream(copier)
        disp.record_stream(copier)
        rgb_host.append(rgb_h)
        disp_host.append(disp_h)
    copier.synchronize()
    return [x.numpy() for x in rgb_host], [x.numpy() for x in disp_host]


def render_rays_sharded(net, rays, batch_size, *, N=128, tn=2, tf=6, u=None, group=None, **kw):
    """Multi-GPU full-image render (BASELINE config 4's data path): every rank
    holds the same ray table [n,6] (any device), renders its contiguous share
    with the HIP path and all-gathers the packed [rgb, disparity] pixels
    (nerf_simple_amd.parallel).  Returns (rgb [n,3] clipped, disparity [n]) on
    every rank's GPU.  Jitter is indexed by global ray id, so the image does
    not depend on the number of ranks."""
    from .. import parallel
    box_mod.refuse_box(kw.get("box"), "the sharded render (render_rays_sharded)")
    dev = next(net.parameters()).device

    def render_fn(r, us, ray_id0):
        return _render_batched(r.to(dev).float().contiguous(), net, batch_size, N, tn, tf,
                               None if us is None else us.to(dev), False, id_base=ray_id0, **kw)

    return parallel.render_image_sharded(rays, render_fn, group=group, u=u)


def _host_pose(pose):
    """pose [4,4] or [3,4] (host tensor / array) as the entry points take it: a contiguous float32 [3,4] numpy copy."""
    import numpy as np
    h_pose = np.zeros((3, 4), dtype=np.float32)
    h_pose[:] = np.asarray(pose, dtype=np.float32)[:3, :4]
    return h_pose


def generate_rays(pose, cam_params, device, ray0=0, n_rays=None):
    """Pinhole rays of an HxW view on the GPU (reference utils/xyz.py:38-52 +
    utils/rendering.py:129-134 run on the CPU): pose [4,4] or [3,4] (host tensor /
    array), cam_params [H,W,f] -> rays [n_rays,6] for pixels ray0.. in row-major
    order."""
    H, W, f = int(cam_params[0]), int(cam_params[1]), float(cam_params[2])
    n = H * W - ray0 if n_rays is None else int(n_rays)
    h_pose = _host_pose(pose)
    rays = torch.empty((n, 6), dtype=torch.float32, device=device)
    _lib.launch("nerf_amd_generate_rays", h_pose.ctypes.data, H, W, f, int(ray0), n, rays, dev=device)
    return rays


def render_view(net, pose, cam_params, *, N=128, tn=2, tf=6, u=None, ray0=0, n_rays=None,
                precision=None, device_rng=False, seed=0, occupancy=None, terminate=None, background=None, controls=None,
                box=None):
    """One view (or the pixel range [ray0, ray0+n_rays) of it) in ONE library
    call: device ray generation -> render_nerf -> clip(rgb,0,1), i.e. the body of
    the reference's per-image loop (utils/rendering.py:139-151) without the
    Python batch loop.  Returns pixels [n,4] = [r,g,b,disparity] on the GPU.
    ``u`` [n,N] explicit jitter for these pixels; default: one CPU
    torch.rand(n,N) like the reference; device_rng=True: counter RNG keyed by
    global pixel id.
    occupancy: an ``OccupancyGrid`` -- the masked render (device ray generation, then the stages of
    utils/occupancy.py); the same conditions as ``render_nerf(..., occupancy=)``: under ``torch.no_grad()``, default
    network shape only.
    terminate: an ``EarlyTermination`` -- early ray termination as in ``render_nerf(..., terminate=)``, on ``occupancy`` or,
    without one, on an all-live grid.
    background: a colour [3] (or one per pixel of the range, [n,3]) behind the volume: pixels = [clip(rgb + (1 - acc)
    background, 0, 1), disparity], the clip behind the blend.  Device ray generation, nerf_amd_render_forward for rgb, disp
    and acc, then one small blend launch (without a background: the one call it was).  Not with occupancy / terminate.
    controls: a ``training.Controls`` -- ``render_nerf``'s: without a grid it stands for ``background``; with ``occupancy`` the
    masked render through the five-output masked compositor (so that acc exists), then the blend and the clip behind it.
    box: a ``SceneBox`` or a ``GridSpan`` -- device ray generation -> the box's positions (nerf_amd_box_positions, jitter keyed by global pixel
    id) -> the render, the background render or the masked / terminated render on the materialised rays under those given
    positions, as the ``occupancy=`` branch already runs; by definition ``render_nerf(generate_rays(...), ..., box=box)`` and
    the clip.  Not inside the one-launch image kernel."""
    box_mod.check_box(box)
    c = controls_mod.from_keywords(controls, {"occupancy": occupancy, "terminate": terminate}, background=background)
    if controls is not None:
        controls_mod.render_only(c, terminate, " (train_step(..., controls=))")
        if c.sigma_noise > 0:
            controls_mod.refuse_noise("render_view trains nothing" if occupancy is None else
                                      "the masked inference render trains nothing")
    dev = next(net.parameters()).device
    if terminate is not None:
        from .occupancy import check_terminable
        check_terminable(terminate, occupancy, net, False)
    elif occupancy is not None:
        from .occupancy import check_renderable
        check_renderable(occupancy, net, False)
    H, W, f = int(cam_params[0]), int(cam_params[1]), float(cam_params[2])
    n = H * W - ray0 if n_rays is None else int(n_rays)
    if not (isinstance(net, Nerf) and net._fused_ok()):
        # a net the fused kernels are not built for (another Nerf(Lp, Ld, H), any module with .forward): device ray
        # generation, then the body of the reference's loop as it stands (render_nerf, clip)
        rays = generate_rays(pose, cam_params, dev, ray0, n)
        with torch.no_grad():
            rgb, disp, _, _, _ = render_nerf(rays, net, N, tn, tf, u=u, outputs=("rgb", "disp", "acc"),
                                             device_rng=device_rng, seed=seed, ray_id0=ray0,
                                             **({} if c is None or c.background is None else {"background": c.background}),
                                             **({} if box is None else {"box": box}))
        return torch.cat([rgb.clamp(0., 1.), disp[:, None]], dim=1)
    c = controls_mod.resolve(c, n, dev, ray0)         # the background, dense or behind the masked render
    code = _lib.precision_of(net, precision)
    net.packed_weights(code)
    rays = None
    if box is not None:
        # the materialised rays, the box's positions on them, then a branch below under NERF_AMD_TS_GIVEN
        box_mod.check_interval(N, tn, tf)
        jitter.check(n, int(N), u=u, shape_error="u must be [n_rays, N]")
        rays = generate_rays(pose, cam_params, dev, ray0, n)
        jit, flags, pending_rng = box_mod.single(box, rays, int(N), tn, tf, u=u, device_rng=device_rng, seed=seed, ray_id0=ray0)
    else:
        # the shape of ``u`` is looked at below, on the masked and background branches only (section 31)
        jit, flags, pending_rng = jitter.single(n, N, dev, u=u, device_rng=device_rng, shape_error=None)
    if pending_rng is not None:
        pending_rng.finish()
    lib = _lib.lib()
    if terminate is not None or occupancy is not None:
        from .occupancy import render_masked, render_terminated
        if jit is not None and tuple(jit.shape) != (n, int(N)):
            raise RuntimeError("u must be [n_rays, N]")
        if rays is None:
            rays = generate_rays(pose, cam_params, dev, ray0, n)
        if terminate is not None:
            return render_terminated(terminate, occupancy, rays, net, int(N), _tbins(tn, tf, N, dev), jit, flags, seed, ray0,
                                     code, (), pixels=True)
        if c is not None:
            return controls_mod.blended(render_masked(occupancy, rays, net, int(N), _tbins(tn, tf, N, dev), jit, flags, seed, ray0,
                                                      code, ()), c, pixels=True)
        return render_masked(occupancy, rays, net, int(N), _tbins(tn, tf, N, dev), jit, flags, seed, ray0, code, (),
                             pixels=True)

    def launch_bg(code, packed):
        return controls_mod.blended(_render_forward(rays, jit, _tbins(tn, tf, N, dev), packed[0], code, flags, seed, ray0, int(N), ()),
                                    c, pixels=True)

    if c is not None:
        if jit is not None and tuple(jit.shape) != (n, int(N)):
            raise RuntimeError("u must be [n_rays, N]")
        if rays is None:
            rays = generate_rays(pose, cam_params, dev, ray0, n)
        return guarded_launch([net], code, launch_bg)
    if box is not None:
        def launch_given(code, packed):       # the render's pixel head on the given positions (render_guided_view's launch)
            pixels = torch.empty((n, 4), dtype=torch.float32, device=dev)
            ws = _lib.workspace(lib.nerf_amd_render_workspace_bytes(code, n, int(N)), dev, floor=0)
            _lib.launch("nerf_amd_render_pixels_forward", rays, jit, None, packed[0], code, flags, int(seed), int(ray0), pixels,
                        ws, n, int(N), dev=dev)
            return pixels

        return guarded_launch([net], code, launch_given)
    h_pose = _host_pose(pose)

    def launch(code, packed):
        pixels = torch.empty((n, 4), dtype=torch.float32, device=dev)
        ws = _lib.workspace(lib.nerf_amd_render_image_workspace_bytes(code, n, N), dev)
        _lib.launch("nerf_amd_render_image_forward", h_pose.ctypes.data, H, W, f, int(ray0), n, jit, _tbins(tn, tf, N, dev),
                    packed[0], code, flags, int(seed), pixels, ws, int(N), dev=dev)
        return pixels

    return guarded_launch([net], code, launch)


def render_view_sharded(net, pose, cam_params, *, group=None, **kw):
    """Multi-GPU render_view: rank r renders its contiguous pixel range and ONE
    all-gather assembles pixels [H*W,4] on every rank (BASELINE config 4)."""
    from .. import parallel
    rank, world = parallel.world_info(group)
    n = int(cam_params[0]) * int(cam_params[1])
    lo, hi = parallel.shard_range(n, rank, world)
    u = kw.pop("u", None)
    bg = kw.get("background")
    if torch.is_tensor(bg) and bg.dim() == 2:            # one colour per pixel of the view: this rank's rows
        kw["background"] = bg[lo:hi]
    shard = render_view(net, pose, cam_params, ray0=lo, n_rays=hi - lo,
                        u=None if u is None else u[lo:hi], **kw)
    return parallel.gather_pixels(shard, n, group)


def sample_pdf(ts, w, Nf, *, u=None, device_rng=False, seed=0, ray_id0=0):
    """Importance sampling for a fine pass (BASELINE config 4; NOT in the
    reference -- parity unpinned, follows the NeRF paper): ts [B,Nc] coarse
    positions, w [B,Nc] coarse weights -> sorted [B,Nc+Nf] positions (the coarse
    ones plus Nf inverse-CDF samples).  u [B,Nf] explicit uniforms; default one
    CPU torch.rand(B,Nf); device_rng=True: counter RNG."""
    _lib.require_cuda_f32(ts, "ts")
    _lib.require_cuda_f32(w, "w")
    B, Nc = ts.shape
    dev = ts.device
    jit, flags, pending_rng = jitter.single(B, Nf, dev, u=u, device_rng=device_rng, shape_error=None)    # u's shape: the caller's
    if pending_rng is not None:
        pending_rng.finish()
    out = torch.empty((B, Nc + Nf), dtype=torch.float32, device=dev)
    _lib.launch("nerf_amd_sample_pdf", ts.contiguous(), w.contiguous(), jit, flags, int(seed), int(ray_id0), out, B, int(Nc),
                int(Nf), dev=dev)
    return out


def _pair_render_controls(controls):
    """``controls=`` of the coarse + fine inference renders, the first thing they look at -> a Controls with a background, or None.
    ``render_nerf``'s rules: TypeError for anything but a Controls, ValueError for a distortion term (a render is no step),
    the regulariser's RuntimeError for sigma noise (an inference render trains nothing)."""
    c = controls_mod.bundle(controls)
    controls_mod.render_only(c)
    if c is not None and c.sigma_noise > 0:
        controls_mod.refuse_noise("the coarse + fine inference render trains nothing")
    return None if c is None or c.background is None else c


def _masked_pair_args(occupancy, net_coarse, net_fine, B, Nc, Nf, u_c, u_f, precision, device_rng, dev):
    """What ``render_hierarchical[_view](..., occupancy=)`` settles before anything is launched or drawn: the grid's and
    the sampler's preconditions, then the jitter (u_c, then u_f, from torch's CPU generator unless given / device_rng).
    -> (precision code, coarse jitter or None, coarse flags, u_f or None)"""
    from .occupancy import check_renderable
    check_renderable(occupancy, net_coarse, False)
    check_renderable(occupancy, net_fine, False)
    _lib.require_pair_sizes(Nc, Nf)
    _lib.require_same_device("occupancy grid", occupancy.words, dev)
    _lib.require_shape(u_c, "u_c", (B, Nc))
    _lib.require_shape(u_f, "u_f", (B, Nf))
    code = _lib.precision_of(net_coarse, precision)
    net_coarse.packed_weights(code)
    net_fine.packed_weights(code)
    return (code,) + jitter.pair(B, Nc, Nf, dev, u_c=u_c, u_f=u_f, device_rng=device_rng)


def render_hierarchical(rays, net_coarse, net_fine, Nc=64, Nf=128, tn=2, tf=6, *, u_c=None, u_f=None,
                        precision=None, device_rng=False, seed=0, ray_id0=0, occupancy=None, box=None, controls=None):
    """Coarse + fine render (BASELINE config 4: 64 + 128 samples).  The reference
    only has the single-pass render_nerf (its CoarseNet / FineNet are empty
    classes), so this composition is new: a coarse render_nerf pass with Nc
    stratified samples, sample_pdf on its weights, and a second render_nerf pass
    of ``net_fine`` on the merged Nc+Nf positions (explicit ts).  Each pass is the
    pinned render_nerf; only the sampler in between is unpinned.
    Returns (fine 5-tuple, coarse 5-tuple, ts_fine).  Every arithmetic step runs in the library
    (sample positions come out of the kernel); see render_hierarchical_view for the one-call form.

    occupancy: ONE ``OccupancyGrid`` masks both passes: masked coarse pass -> sample_pdf on its
    weights (exactly 0 at a dead sample; a ray with no live coarse sample gets uniform fine samples) -> masked fine pass
    on the merged positions; each network sees live samples only, two host synchronisations per call, both passes at one
    precision under one range guard.  Inference only (``torch.no_grad()``), default network shape only.
    box: refused (RuntimeError before anything is drawn): the scene box serves the single-network renders.
    controls: a ``training.Controls`` with a background, with or without ``occupancy``: ``rgb`` of the
    fine and of the coarse 5-tuple becomes rgb + (1 - acc) background through nerf_amd_background_blend; every other output,
    ``ts_fine`` included, is bit for bit what it was.  ``controls.sigma_noise > 0`` raises RuntimeError (a regulariser: this
    render trains nothing), a non-zero ``controls.distortion`` ValueError."""
    c = _pair_render_controls(controls)
    box_mod.refuse_box(box, "the coarse + fine pair (render_hierarchical)")
    _lib.require_cuda_f32(rays, "rays")
    dev, B = rays.device, rays.size(0)
    if c is not None:
        c = controls_mod.resolve(c, _lib.require_rays(rays), dev, ray_id0)        # the background's shape: before anything is drawn
        fine, coarse, ts_f = render_hierarchical(rays, net_coarse, net_fine, Nc, Nf, tn, tf, u_c=u_c, u_f=u_f, precision=precision,
                                                 device_rng=device_rng, seed=seed, ray_id0=ray_id0, occupancy=occupancy)
        return controls_mod.blended(fine, c), controls_mod.blended(coarse, c), ts_f
    if occupancy is not None:
        from .occupancy import render_masked_pair
        _lib.require_rays(rays)
        Nc, Nf = int(Nc), int(Nf)
        if torch.is_grad_enabled() and rays.requires_grad:
            raise RuntimeError("the masked render (occupancy=) is inference only: call it under torch.no_grad()")
        code, jit, flags, u_f = _masked_pair_args(occupancy, net_coarse, net_fine, B, Nc, Nf, u_c, u_f, precision, device_rng, dev)
        rays = rays.detach().contiguous()
        tb = _tbins(tn, tf, Nc, dev)
        from .xyz import range_check_rays
        range_check_rays(rays, jit, tb, flags, seed, ray_id0, Nc)
        with torch.no_grad():
            return render_masked_pair(occupancy, rays, net_coarse, net_fine, Nc, Nf, tb, jit, flags, u_f, device_rng, seed,
                                      ray_id0, code)
    rays = rays.detach().contiguous()
    code = _lib.precision_of(net_coarse, precision)
    net_coarse.packed_weights(code)
    # the coarse half of the pair rule; ``sample_pdf`` below settles u_f behind the coarse pass (the same draw order)
    jit, flags, pending_rng = jitter.single(B, Nc, dev, u=u_c, device_rng=device_rng, names=("u_c", None), shape_error=None)
    if pending_rng is not None:
        pending_rng.finish()
    # the coarse pass through the stage-1 entry point: the sampler needs the positions the kernel drew
    def launch(code, packed):
        raw = torch.empty((B, Nc, 4), dtype=torch.float32, device=dev)
        ts_c = torch.empty((B, Nc), dtype=torch.float32, device=dev)
        outs = [torch.empty(s_, dtype=torch.float32, device=dev) for s_ in ((B, 3), (B,), (B, Nc), (B,), (B, Nc))]
        _lib.launch("nerf_amd_mlp_forward_rays", rays, jit, _tbins(tn, tf, Nc, dev), packed[0], code, flags, int(seed),
                    int(ray_id0), raw, ts_c, B, Nc, dev=dev)
        _lib.launch("nerf_amd_volume_render_rays", raw, ts_c, rays, *outs, B, Nc, dev=dev)
        return ts_c, tuple(outs)

    ts_c, coarse = guarded_launch([net_coarse], code, launch)
    ts_f = sample_pdf(ts_c, coarse[4], Nf, u=u_f, device_rng=device_rng, seed=seed, ray_id0=ray_id0)
    fine = render_nerf(rays, net_fine, Nc + Nf, tn, tf, ts=ts_f, precision=precision)
    return fine, coarse, ts_f


def render_hierarchical_view(net_coarse, net_fine, pose, cam_params, Nc=64, Nf=128, *, tn=2, tf=6, u_c=None, u_f=None,
                             ray0=0, n_rays=None, precision=None, device_rng=False, seed=0, occupancy=None, box=None,
                             controls=None):
    """BASELINE config 4 for one view (or its pixel range [ray0, ray0+n_rays)) in ONE library call:
    device ray generation -> coarse pass (Nc stratified samples) -> sample_pdf -> fine pass on the
    Nc+Nf merged positions -> clip(rgb,0,1)  (nerf_amd_render_hierarchical_forward: four launches,
    no torch arithmetic on the path).  Returns pixels [n,4] = [r,g,b,disparity] on the GPU.
    u_c [n,Nc] / u_f [n,Nf]: explicit uniforms for these pixels; default: the reference-style CPU
    draws torch.rand(n,Nc) then torch.rand(n,Nf); device_rng=True: counter RNG keyed by global pixel id.
    Parity unpinned (no reference counterpart).
    occupancy: an ``OccupancyGrid`` for both passes -- device ray generation, then the composition of
    ``render_hierarchical(..., occupancy=)``, then the clip (not one library call: two host reads, one per pass).
    box: refused (RuntimeError before anything is drawn).
    controls: a ``training.Controls`` with a background -- device ray generation, the composition of
    ``render_hierarchical(..., controls=)`` on those rays (jitter ids from ``ray0``), then clip(rgb + (1 - acc) background,
    0, 1) beside the fine disparity (the clip behind the blend).  Sigma noise / a distortion term: as ``render_hierarchical``.
    Without it the dense call stays the one library call it is."""
    c = _pair_render_controls(controls)
    box_mod.refuse_box(box, "the coarse + fine pair (render_hierarchical_view)")
    dev = next(net_coarse.parameters()).device
    H, W, f = int(cam_params[0]), int(cam_params[1]), float(cam_params[2])
    n = H * W - ray0 if n_rays is None else int(n_rays)
    if device_rng:
        u_c = u_f = None                 # this entry point's own rule (section 31): device_rng drops given uniforms
    if c is not None:
        c = controls_mod.resolve(c, n, dev, ray0)               # the background's shape: before anything is drawn
        _lib.require_shape(u_c, "u_c", (n, int(Nc)))
        _lib.require_shape(u_f, "u_f", (n, int(Nf)))
        rays = generate_rays(pose, cam_params, dev, ray0, n)
        with torch.no_grad():
            fine = render_hierarchical(rays, net_coarse, net_fine, Nc, Nf, tn, tf, u_c=u_c, u_f=u_f, precision=precision,
                                       device_rng=device_rng, seed=seed, ray_id0=ray0, occupancy=occupancy)[0]
        return controls_mod.blended(fine, c, pixels=True)
    if occupancy is not None:
        from .occupancy import render_masked_pair
        Nc, Nf = int(Nc), int(Nf)
        code, jit, flags, u_f = _masked_pair_args(occupancy, net_coarse, net_fine, n, Nc, Nf, u_c, u_f, precision, device_rng, dev)
        rays = generate_rays(pose, cam_params, dev, ray0, n)
        with torch.no_grad():
            return render_masked_pair(occupancy, rays, net_coarse, net_fine, Nc, Nf, _tbins(tn, tf, Nc, dev), jit, flags, u_f,
                                      device_rng, seed, ray0, code, pixels=True)[0]
    code = _lib.precision_of(net_coarse, precision)
    u_c, flags, u_f = jitter.pair(n, Nc, Nf, dev, u_c=u_c, u_f=u_f, device_rng=device_rng)
    lib, h_pose = _lib.lib(), _host_pose(pose)

    def launch(code, packed):
        pixels = torch.empty((n, 4), dtype=torch.float32, device=dev)
        ws = _lib.workspace(lib.nerf_amd_render_hierarchical_workspace_bytes(n, Nc, Nf), dev)
        _lib.launch("nerf_amd_render_hierarchical_forward", h_pose.ctypes.data, H, W, f, int(ray0), n, u_c, u_f,
                    _tbins(tn, tf, Nc, dev), packed[0], packed[-1], code, flags, int(seed), pixels, ws, int(Nc), int(Nf), dev=dev)
        return pixels

    # one precision for both passes: if either network left the fp16 range, both render with bf16 operands
    return guarded_launch([net_coarse] if net_fine is net_coarse else [net_coarse, net_fine], code, launch)


def render_hierarchical_sharded(net_coarse, net_fine, pose, cam_params, Nc=64, Nf=128, *, group=None, **kw):
    """Multi-GPU config 4: rank r renders its contiguous pixel range coarse+fine in one library call and
    ONE all-gather assembles pixels [H*W,4] on every rank.  Jitter is keyed by global pixel id
    (device RNG) or sliced from the caller's u_c / u_f, so the image does not depend on the world size."""
    from .. import parallel
    rank, world = parallel.world_info(group)
    n = int(cam_params[0]) * int(cam_params[1])
    lo, hi = parallel.shard_range(n, rank, world)
    u_c, u_f = kw.pop("u_c", None), kw.pop("u_f", None)
    shard = render_hierarchical_view(net_coarse, net_fine, pose, cam_params, Nc, Nf, ray0=lo, n_rays=hi - lo,
                                     u_c=None if u_c is None else u_c[lo:hi], u_f=None if u_f is None else u_f[lo:hi],
                                     **kw)
    return parallel.gather_pixels(shard, n, group)


def _check_guided(net, proposal):
    """The guided renders' and steps' limits, checked before anything is drawn or launched."""
    from .proposal import ProposalVolume
    if not isinstance(proposal, ProposalVolume):
        raise TypeError("proposal must be a ProposalVolume (utils/proposal.py)")
    if not (isinstance(net, Nerf) and net._fused_ok()):
        raise RuntimeError("guided sampling serves the default Nerf(10, 4, 256) only: other network sizes and foreign nets "
                           "are not supported; nothing falls back")


def render_guided(rays, net, Nc, Nf, proposal, tn=2, tf=6, *, u_c=None, ts_c=None, u_f=None, outputs=ALL_OUTPUTS,
                  precision=None, device_rng=False, seed=0, ray_id0=0, occupancy=None, box=None):
    """Grid-guided render: ONE network on Nc + Nf positions per ray, the Nf new ones placed by
    ``proposal`` (a ``ProposalVolume``, utils/proposal.py) from its sigma volume instead of by a coarse network.  It is
    ``render_nerf(rays, net, Nc + Nf, ts=proposal.sample(rays, Nc, Nf, ...))``; jitter arguments as ``ProposalVolume.sample``
    (default: ``render_hierarchical``'s two CPU draws).  Returns render_nerf's five outputs plus ts [B, Nc + Nf].  Default
    network shape only; no gradients to the rays; no host synchronisation beyond the fp16 range guard's.

    occupancy: an ``OccupancyGrid`` -- the masked guided render: the masked guided placement (dead
    coarse samples weigh nothing; the merged positions come back marked) and the masked render on those positions under
    that mark, which is not formed a second time.  By definition ``render_nerf(rays, net, Nc + Nf, ts=ts, occupancy=occupancy)``
    on the placement's ``ts``; inference only (call it under ``torch.no_grad()``), one host synchronisation, sets
    ``occupancy.last_stats``.
    box: refused (RuntimeError before anything is drawn): the guided placement has its own interval."""
    box_mod.refuse_box(box, "the guided render (render_guided)")
    _check_guided(net, proposal)
    if occupancy is not None:
        return _render_guided_masked(rays, net, Nc, Nf, proposal, tn, tf, u_c, ts_c, u_f, outputs, precision, device_rng, seed,
                                     ray_id0, occupancy)
    B, Nc, Nf = proposal.check(rays, Nc, Nf, u_c, ts_c, u_f, device_rng)
    if not (torch.is_grad_enabled() and any(p.requires_grad for p in net.parameters())):
        net.packed_weights(_lib.precision_of(net, precision))     # errors before the draws
    ts = proposal.sample(rays, Nc, Nf, tn, tf, u_c=u_c, ts_c=ts_c, u_f=u_f, device_rng=device_rng, seed=seed, ray_id0=ray_id0)
    return render_nerf(rays, net, Nc + Nf, tn, tf, ts=ts, outputs=outputs, precision=precision) + (ts,)


def _render_guided_masked(rays, net, Nc, Nf, proposal, tn, tf, u_c, ts_c, u_f, outputs, precision, device_rng, seed, ray_id0,
                          occupancy):
    """The body of ``render_guided(..., occupancy=)``: render_nerf's masked branch on the placement's positions and mark."""
    from .occupancy import check_renderable, _render_marked
    from .xyz import range_check_rays
    check_renderable(occupancy, net, torch.is_tensor(rays) and rays.requires_grad)
    proposal.check(rays, Nc, Nf, u_c, ts_c, u_f, device_rng, occupancy=occupancy)
    code = _lib.precision_of(net, precision)
    net.packed_weights(code)                      # errors before the draws
    with torch.no_grad():
        rays = rays.detach().contiguous()
        ts, mark = proposal.sample(rays, Nc, Nf, tn, tf, u_c=u_c, ts_c=ts_c, u_f=u_f, device_rng=device_rng, seed=seed,
                                   ray_id0=ray_id0, occupancy=occupancy, return_mark=True)
        range_check_rays(rays, ts, None, _lib.FLAG_TS_GIVEN, 0, 0, ts.size(1))
        return _render_marked(occupancy, rays, net, ts, mark, code, outputs) + (ts,)


def render_guided_view(net, pose, cam_params, Nc, Nf, proposal, *, tn=2, tf=6, u_c=None, u_f=None, ray0=0, n_rays=None,
                       precision=None, device_rng=False, seed=0, occupancy=None, box=None):
    """One view (or its pixel range [ray0, ray0 + n_rays)) through the grid-guided render: device ray generation ->
    ``proposal.sample`` (counter RNG keyed by global pixel id with device_rng=True) -> the fused render on the given
    positions -> clip(rgb, 0, 1).  Returns pixels [n, 4] = [r, g, b, disparity] on the GPU.  u_c [n, Nc] / u_f [n, Nf]:
    explicit uniforms for these pixels; default: the CPU draws torch.rand(n, Nc) then torch.rand(n, Nf).

    occupancy: an ``OccupancyGrid`` -- device ray generation -> the masked guided placement -> the
    masked render's pixel head (nerf_amd_volume_render_masked_pixels) on its positions under its mark; under
    ``torch.no_grad()``, one host synchronisation.
    box: refused (RuntimeError before anything is drawn)."""
    box_mod.refuse_box(box, "the guided render (render_guided_view)")
    _check_guided(net, proposal)
    if occupancy is not None:
        from .occupancy import check_renderable
        check_renderable(occupancy, net, False)
    dev = next(net.parameters()).device
    n = int(cam_params[0]) * int(cam_params[1]) - ray0 if n_rays is None else int(n_rays)
    code = _lib.precision_of(net, precision)
    net.packed_weights(code)
    rays = generate_rays(pose, cam_params, dev, ray0, n)
    if occupancy is not None:
        # the masked guided placement -> the masked render's pixel head on its positions under its mark (section 24)
        from .occupancy import _render_marked
        with torch.no_grad():
            ts, mark = proposal.sample(rays, Nc, Nf, tn, tf, u_c=u_c, u_f=u_f, device_rng=device_rng, seed=seed, ray_id0=ray0,
                                       occupancy=occupancy, return_mark=True)
            return _render_marked(occupancy, rays, net, ts, mark, code, (), pixels=True)
    ts = proposal.sample(rays, Nc, Nf, tn, tf, u_c=u_c, u_f=u_f, device_rng=device_rng, seed=seed, ray_id0=ray0)
    N, lib = ts.size(1), _lib.lib()

    def launch(code, packed):
        pixels = torch.empty((n, 4), dtype=torch.float32, device=dev)
        ws = _lib.workspace(lib.nerf_amd_render_workspace_bytes(code, n, N), dev, floor=0)
        _lib.launch("nerf_amd_render_pixels_forward", rays, ts, None, packed[0], code, _lib.FLAG_TS_GIVEN, int(seed), int(ray0),
                    pixels, ws, n, N, dev=dev)
        return pixels

    with torch.no_grad():
        return guarded_launch([net], code, launch)
