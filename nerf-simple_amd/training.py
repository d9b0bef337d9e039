"""Training-side entry points: the step of reference train.py:47-57 on the GPU.

What runs where in a training step (BASELINE config 5); every stage is a hand-written HIP kernel
behind the C ABI, torch supplies tensors, streams, autograd bookkeeping and the collective:

  sampling + encoding + 12 dense layers, forward    nerf_amd_mlp_forward_train (the fused inference
                                                    kernel, also saving point-blocked bf16 activations
                                                    and ReLU mask bit planes)
  sigma -> alpha compositing, forward               nerf_amd_volume_render
  MSE loss and its gradient                         nerf_amd_mse_loss
  compositing, backward (suffix-sum scan)           nerf_amd_volume_render_backward
  distortion loss on the weights (distortion=)      nerf_amd_distortion_loss + nerf_amd_sum_f32
  dense layers, backward dX chain (on-chip)         nerf_amd_mlp_backward
  dense layers, dW = dY^T X and db = sum dY         nerf_amd_param_gradients (one split-K launch for
                                                    all 14 products into ONE flat gradient vector)
  gradient exchange                                 RCCL all-reduce of that flat vector, in place (parallel.py)
  optimizer                                         optim.FusedAdam (one launch + re-pack) or
                                                    torch.optim.Adam (reference train.py:43)
  the whole step as captured hipGraphs              GraphedTrainStep (below)

Precision: the fused training kernels exist in bf16 only (gradients need bf16's exponent range; fp16
would need loss scaling).  A module built with precision='bf16' or 'fp16' trains through them --
``precision`` selects the INFERENCE kernel only.  precision='fp32' trains EXACTLY, as the reference does
(fp32 weights, activations and gradients: utils/generic_mlp.py, every nn.Linear and its backward on the
strided fp32 MFMA GEMM nerf_amd_linear_f32, layer by layer): the slow path, exact to fp32 round-off -- its gradients match
the reference's autograd to 1e-5; long dW / db reductions are summed with float atomics, so the last bits vary from run to run -- for checks and small problems; GraphedTrainStep is the fused bf16 step only.
"""

import torch

from . import _lib
from .utils import controls as controls_mod
from .utils.controls import FINE_NOISE_OFFSET, Background as _Background, Controls       # noqa: F401  (the public names)
from .utils.jitter import tbins as _tbins
from .utils.rendering import ALL_OUTPUTS, _check_guided, _five_outputs, _render_generic, _render_nerf, sample_pdf


def img_mse(gt, pred):
    """mean((pred - gt)^2)  (reference train.py:16-19)."""
    if not torch.is_tensor(gt):
        gt = torch.from_numpy(gt).float()
    return torch.mean((pred - gt) ** 2)


def img_psnr(gt, pred):
    """20 log10(max(gt)) - 10 log10(mse): the peak is max(gt), not 1.0
    (reference train.py:21-26)."""
    if not torch.is_tensor(gt):
        gt = torch.from_numpy(gt).float()
    ten = torch.tensor(10.0)
    return 20 * torch.log(torch.max(gt)) / torch.log(ten) - 10 * torch.log(img_mse(gt, pred)) / torch.log(ten)


# --------------------------------------------------------------------------
# MSELoss with the HIP kernel (value and gradient in one launch)
# --------------------------------------------------------------------------
class _MseLoss(torch.autograd.Function):
    """nn.MSELoss()(pred, target) (reference train.py:42,52: mean over all elements) through
    nerf_amd_mse_loss: one launch writes the loss and 2 (pred - target) / n."""

    @staticmethod
    def forward(ctx, pred, target):
        pred, target = pred.contiguous(), target.contiguous()
        if pred.shape != target.shape:
            raise RuntimeError(f"mse_loss: shapes {tuple(pred.shape)} and {tuple(target.shape)} differ")
        dev = pred.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        g_pred = torch.empty_like(pred)
        _lib.launch("nerf_amd_mse_loss", pred, target, loss, g_pred, pred.numel(), dev=dev)
        ctx.save_for_backward(g_pred)
        return loss

    @staticmethod
    def backward(ctx, g):
        (g_pred,) = ctx.saved_tensors
        return g_pred * g, None


def mse_loss(pred, target):
    """criterion(rgb, gt_colors) of reference train.py:42,52 on device tensors (fp32)."""
    _lib.require_cuda_f32(pred, "pred")
    _lib.require_cuda_f32(target, "target")
    return _MseLoss.apply(pred, target.detach())


# --------------------------------------------------------------------------
# compositor with a HIP backward
# --------------------------------------------------------------------------
def _grad_arg(g):
    """An upstream gradient as the backward kernels take it: fp32 contiguous, or None for a missing or empty one"""
    return None if (g is None or g.numel() == 0) else g.contiguous().float()


class _VolumeRender(torch.autograd.Function):
    """volume_render with the HIP backward.  ``from_rays``: ``dirs`` is the [B,6] ray table and the
    kernels normalise rays[:,3:] themselves (render_nerf, utils/rendering.py:37,43)."""

    @staticmethod
    def forward(ctx, raw, ts, dirs, from_rays):
        B, N = raw.shape[0], raw.shape[1]
        dev = raw.device
        raw, ts, dirs = raw.contiguous(), ts.contiguous(), dirs.contiguous()
        rgb, disp, alpha, acc, w = _five_outputs(B, N, ALL_OUTPUTS, dev)
        if from_rays:
            _lib.launch("nerf_amd_volume_render_rays", raw, ts, dirs, rgb, disp, alpha, acc, w, B, N, dev=dev)
        else:
            _lib.launch("nerf_amd_volume_render", raw, ts, dirs, 3, rgb, disp, alpha, acc, w, B, N, dev=dev)
        ctx.save_for_backward(raw, ts, dirs)
        ctx.from_rays = from_rays
        if N == 1:        # the reference's empty sample axis (utils/rendering.py:60-61; csrc/composite_device.h)
            alpha, w = alpha[:, :0], w[:, :0]
        return rgb, disp, alpha, acc, w

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_alpha, g_acc, g_w):
        raw, ts, dirs = ctx.saved_tensors
        B, N = raw.shape[0], raw.shape[1]
        dev = raw.device
        d_raw = torch.empty_like(raw)
        g_rgb, g_disp, g_alpha, g_acc, g_w = map(_grad_arg, (g_rgb, g_disp, g_alpha, g_acc, g_w))
        if ctx.from_rays:
            _lib.launch("nerf_amd_volume_render_rays_backward", raw, ts, dirs, g_rgb, g_disp, g_alpha, g_acc, g_w, d_raw, B, N,
                        dev=dev)
        else:
            _lib.launch("nerf_amd_volume_render_backward", raw, ts, dirs, 3, g_rgb, g_disp, g_alpha, g_acc, g_w, d_raw, B, N,
                        dev=dev)
        return d_raw, None, None, None


def volume_render_autograd(nerf_outs, ts, dirs):
    """volume_render (reference utils/rendering.py:47-85) with gradients to
    nerf_outs; ts and dirs get none (they carry none in the reference either)."""
    return _VolumeRender.apply(nerf_outs.float(), ts.detach(), dirs.detach(), False)


# --------------------------------------------------------------------------
# the two training controls around the dense compositor
# --------------------------------------------------------------------------
class _SigmaNoise(torch.autograd.Function):
    """raw [B,N,4] -> the same with sigma' = sigma + std z in column 3 (nerf_amd_sigma_noise; the reference's
    `## TODO add gaussian noise regularizer`, utils/rendering.py:63).  d sigma' / d sigma = 1: the backward is the identity."""

    @staticmethod
    def forward(ctx, raw, std, noise_seed, ray_id0):
        B, N = raw.shape[0], raw.shape[1]
        dev = raw.device
        raw = raw.contiguous()
        out = torch.empty_like(raw)
        _lib.launch("nerf_amd_sigma_noise", raw, out, float(std), 0, int(noise_seed) & (2 ** 64 - 1), None, int(ray_id0), B, N,
                    dev=dev)
        return out

    @staticmethod
    def backward(ctx, g):
        return g, None, None, None


def composite_with_controls(raw, ts, dirs, from_rays, c, masked=None):
    """The one place the controls are applied with gradients: noise on the raw density -> the compositor -> ``w.ts`` = the sample
    positions (what a distortion term on w needs beside it) -> the blend.  ``c``: a ``Resolved`` or None.
    Two heads.  Dense: _VolumeRender(raw [B,N,4], ts, dirs, from_rays) behind _SigmaNoise.  Masked (``masked`` = the (head, B, N) of
    _MaskedVolumeRender): raw is raw_live [P',4], the noise is _MaskedSigmaNoise's, and ``ts`` is None (``w.ts`` is not set) or a
    callable that forms the positions, called behind the compositor."""
    if c is not None and c.std:
        raw = (_SigmaNoise.apply(raw, c.std, c.noise_seed, c.noise_ray_id0) if masked is None else
               _MaskedSigmaNoise.apply(raw, c.std, c.noise_seed, c.noise_ray_id0, masked[0][6:8] + masked[1:]))
    out = _VolumeRender.apply(raw, ts, dirs, from_rays) if masked is None else _MaskedVolumeRender.apply(raw, *masked)
    if ts is not None:
        out[4].ts = ts() if callable(ts) else ts
    if c is not None and c.bg is not None:
        out = (_Background.apply(out[0], out[3], c.bg, c.stride),) + tuple(out[1:])
    return out


# --------------------------------------------------------------------------
# the distortion loss on the compositor's weights
# --------------------------------------------------------------------------
def _distortion_launch(w, ts, t_far, coef, want_loss, want_grad):
    """nerf_amd_distortion_loss on w [B,N], ts [B,N]: (coef D per ray [B], coef dD/dw [B,N]); the reference's empty sample
    axis (w [B,0] at N == 1) has D = 0 and no gradient."""
    _lib.require_cuda_f32(w, "w")
    _lib.require_cuda_f32(ts, "ts")
    B, dev = ts.shape[0], ts.device
    if w.dim() != 2 or ts.dim() != 2 or w.shape[0] != B or (tuple(w.shape) != tuple(ts.shape) and not (w.shape[1] == 0 and ts.shape[1] == 1)):
        raise RuntimeError(f"distortion loss: w {tuple(w.shape)} and ts {tuple(ts.shape)} must both be [B, N]")
    if w.shape[1] == 0:
        return torch.zeros((B,), dtype=torch.float32, device=dev), torch.zeros_like(w)
    w, ts = w.contiguous(), ts.contiguous()
    loss_ray = torch.empty((B,), dtype=torch.float32, device=dev) if want_loss else None
    g_w = torch.empty_like(w) if want_grad else None
    _lib.launch("nerf_amd_distortion_loss", ts, w, float(t_far), float(coef), loss_ray, g_w, B, w.shape[1], dev=dev)
    return loss_ray, g_w


class _DistortionRays(torch.autograd.Function):
    """w [B,N] -> coef D per ray [B] through nerf_amd_distortion_loss, which writes coef dD/dw in the same launch."""

    @staticmethod
    def forward(ctx, w, ts, t_far, coef):
        loss_ray, g_w = _distortion_launch(w, ts, t_far, coef, True, True)
        ctx.save_for_backward(g_w)
        return loss_ray

    @staticmethod
    def backward(ctx, g):
        (g_w,) = ctx.saved_tensors
        return g_w * g[:, None], None, None, None


class _DistortionTerm(torch.autograd.Function):
    """w [B,N] -> the step's scalar term sum_rays coef D: nerf_amd_distortion_loss, then nerf_amd_sum_f32 on its per-ray values
    (one workgroup, fixed order) -- the two launches a graphed step's head and side branch make of it."""

    @staticmethod
    def forward(ctx, w, ts, t_far, coef):
        loss_ray, g_w = _distortion_launch(w, ts, t_far, coef, True, True)
        dev = loss_ray.device
        term = torch.zeros((), dtype=torch.float32, device=dev)
        if loss_ray.numel():
            _lib.launch("nerf_amd_sum_f32", loss_ray, term, loss_ray.numel(), dev=dev)
        ctx.save_for_backward(g_w)
        return term

    @staticmethod
    def backward(ctx, g):
        (g_w,) = ctx.saved_tensors
        return g_w * g, None, None, None


def distortion_loss(w, ts, tn=2, tf=6):
    """mip-NeRF 360's distortion loss of each ray's compositing weights ``w`` [B,N] at the positions ``ts`` [B,N] (nondecreasing
    along a ray; they carry no gradient), on the normalised distance: D / (tf - tn) per ray, [B], differentiable in ``w``.
    Sample i owns [t_i, t_{i+1}], the last one [t_{N-1}, tf] (include/nerf_amd.h nerf_amd_distortion_loss); O(N) per ray."""
    return _DistortionRays.apply(w, ts.detach(), float(tf), 1.0 / (float(tf) - float(tn)))


def _distortion_coef(lam, B, tn, tf):
    """lambda / (B (tf - tn)) in float64; the launch rounds it to fp32 once."""
    return float(lam) / (float(B) * (float(tf) - float(tn)))


def _distortion_term(w, ts, lam, tn, tf):
    """lambda / (B (tf - tn)) sum_rays D as a 0-d tensor, differentiable in ``w``."""
    if ts is None:
        raise RuntimeError("distortion: this render did not hand back its sample positions (the net does not train)")
    return _DistortionTerm.apply(w, ts.detach(), float(tf), _distortion_coef(lam, ts.shape[0], tn, tf))


# --------------------------------------------------------------------------
# fused dense layers: HIP forward (saving activations) + HIP dX chain + HIP dW
# --------------------------------------------------------------------------
def _check_fused_trainable(precision):
    if _lib.precision_code(precision) == _lib.F32:
        raise RuntimeError("the fused training step is bf16 (NERF_AMD_EUNSUP for precision='fp32'): build the module with "
                           "precision='bf16' (or 'fp16': bf16 training, fp16 inference), or train the fp32 module with "
                           "training.train_step (exact, layer by layer)")


class _FusedDense(torch.autograd.Function):
    """(rays, jitter) -> raw [B,N,4], ts [B,N]  -- or, with ``rays`` None, points v [P,6] -> raw [P,1,4] --
    through nerf_amd_mlp_forward_train[_points]; backward: nerf_amd_mlp_backward for every layer's
    pre-activation gradient, then nerf_amd_param_gradients (split-K GEMMs + column sums) into ONE flat
    fp32 vector in state_dict order, handed back to autograd as 24 views.

    Gradients to the inputs (``rays`` or ``pts`` requiring grad: pose refinement, iNeRF) come from
    nerf_amd_input_gradients on the same dY.  Only what autograd asks for is computed: with no parameter
    needing a gradient the encoder rows and the dW products are skipped, with no input needing one
    nothing beyond the parameter path is launched."""

    @staticmethod
    def forward(ctx, net, rays, jit, tbins, flags, seed, ray_id0, N, pts, *params):
        lib = _lib.lib()
        src = rays if rays is not None else pts
        B, dev = src.size(0), src.device
        P = B * N
        # a diverged run is loud: the status words of the previous forwards (non-finite activations / weights) are
        # looked at here, without waiting (_StatusWatch below; the graphed step does the same)
        watch = net.__dict__.get("_watch")
        if watch is None:
            watch = net.__dict__["_watch"] = _StatusWatch()
            net.__dict__["_watch_calls"] = 0
        watch.raise_if_diverged("forward")
        packed = net.packed_weights(_lib.BF16)
        need_w = any(ctx.needs_input_grad[9:])
        need_in = ctx.needs_input_grad[1] or ctx.needs_input_grad[8]
        raw = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
        ts = torch.empty((B, N), dtype=torch.float32, device=dev)
        acts = torch.empty(int(lib.nerf_amd_train_activation_bytes(P)), dtype=torch.uint8, device=dev)
        # the bf16 encoder rows are operands of the dW products only
        posx = torch.empty((P, 64) if need_w else (0,), dtype=torch.bfloat16, device=dev)
        posd = torch.empty((P, 32) if need_w else (0,), dtype=torch.bfloat16, device=dev)
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            if rays is not None:
                _lib.launch("nerf_amd_mlp_forward_train", rays, jit, tbins, packed, flags, int(seed), int(ray_id0), raw, ts,
                            acts, B, N, stream=st)
                # encoder outputs in the reference's column order: the inputs of the dW products of
                # layers_0.0 / skip_conn_layer / color_fc.0 (same sample positions: ts given)
                if need_w:
                    _lib.launch("nerf_amd_sample_encode_bf16", rays, ts, None, _lib.FLAG_TS_GIVEN, 0, 0, posx, posd, None, B, N,
                                stream=st)
            else:
                _lib.launch("nerf_amd_mlp_forward_train_points", pts, packed, raw, acts, P, stream=st)
                if need_w:
                    _lib.launch("nerf_amd_encode_points_bf16", pts, posx, posd, P, stream=st)
        net.__dict__["_watch_calls"] += 1
        watch.push(packed, net.__dict__["_watch_calls"])
        ctx.net, ctx.P, ctx.N = net, P, N
        ctx.shapes = [tuple(p.shape) for p in params]
        ctx.need_w, ctx.need_in = need_w, need_in
        # the input gradient reads the forward's weights (fp32, state_dict order) and its inputs: the points, or the
        # rays and the sample positions the forward drew
        wflat = torch.cat([p.detach().reshape(-1).float() for p in params]) if need_in else None
        ctx.save_for_backward(acts, posx, posd, wflat, src if need_in else None, ts if need_in else None)
        ctx.rays_mode = rays is not None
        ctx.mark_non_differentiable(ts)
        return raw, ts

    @staticmethod
    def backward(ctx, g_raw, _g_ts):
        lib = _lib.lib()
        acts, posx, posd, wflat, src, ts = ctx.saved_tensors
        net, P = ctx.net, ctx.P
        dev = acts.device
        g = g_raw.reshape(P, 4).contiguous().float()
        image = net.packed_weights(_lib.BF16_BWD)
        dys = torch.empty_like(acts)
        d_in = None
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            _lib.launch("nerf_amd_mlp_backward", g, image, acts, dys, P, stream=st)
            if ctx.need_in:
                dv = torch.empty((P, 6), dtype=torch.float32, device=dev)
                if ctx.rays_mode:
                    d_in = torch.empty((P // ctx.N, 6), dtype=torch.float32, device=dev)
                    _lib.launch("nerf_amd_input_gradients", dys, wflat, None, src, ts, dv, d_in, P, ctx.N, stream=st)
                else:
                    d_in = dv
                    _lib.launch("nerf_amd_input_gradients", dys, wflat, src, None, None, dv, None, P, 1, stream=st)
            if ctx.need_w:
                flat = torch.empty(int(lib.nerf_amd_param_count()), dtype=torch.float32, device=dev)
                scratch = torch.empty(max(int(lib.nerf_amd_param_gradients_scratch_bytes(P)), 16), dtype=torch.uint8,
                                      device=dev)
                _lib.launch("nerf_amd_param_gradients", g, acts, dys, posx, posd, scratch, flat, P, stream=st)
        grads, off = [], 0
        for shp in ctx.shapes:
            n = 1
            for s_ in shp:
                n *= s_
            grads.append(flat[off:off + n].view(shp) if ctx.need_w else None)
            off += n
        d_rays = d_in if ctx.rays_mode else None
        d_pts = None if ctx.rays_mode else d_in
        return (None, d_rays) + (None,) * 6 + (d_pts,) + tuple(grads)


def nerf_forward_autograd(net, v, precision):
    """Nerf.forward (reference utils/nets.py:34-43) with gradients to the parameters and / or to v: the fused
    training forward on points, v [P,6] -> [P,4] (precision 'fp32': the exact layer-by-layer path)."""
    if _lib.precision_code(precision) == _lib.F32:
        from .utils import generic_mlp
        return generic_mlp.forward(net, v)
    params = [p for _, p in net.named_parameters()]
    raw, _ = _FusedDense.apply(net, None, None, None, 0, 0, 0, 1, v.contiguous(), *params)
    return raw.reshape(-1, 4)


def render_nerf_autograd(rays, net, N, tn, tf, jit, flags, precision, seed, ray_id0, c=None):
    """render_nerf (reference utils/rendering.py:13-45) with gradients to the
    parameters of ``net`` and, when ``rays`` requires grad, to the rays; returns the same 5-tuple.
    ``c``: the ``Resolved`` controls of ``composite_with_controls``, None = none."""
    if _lib.precision_code(precision) == _lib.F32:
        # exact fp32: the reference's own composition (sampling -> net.forward -> volume_render), each stage a HIP kernel
        from .utils import generic_mlp

        class _Exact:
            @staticmethod
            def forward(q):
                return generic_mlp.forward(net, q)

        return _render_generic(rays, _Exact, N, tn, tf, jit, flags, ALL_OUTPUTS, seed, ray_id0, c)
    dev = rays.device
    params = [p for _, p in net.named_parameters()]
    raw, ts = _FusedDense.apply(net, rays, jit, _tbins(tn, tf, N, dev), flags, seed, ray_id0, N, None, *params)
    # the compositor's |d_hat| factor carries no gradient (|d_hat| == 1): the rays enter it detached
    return composite_with_controls(raw, ts, rays.detach(), True, c)


# --------------------------------------------------------------------------
# training with empty-space skipping: the masked render with gradients
# --------------------------------------------------------------------------
class _MaskedVolumeRender(torch.autograd.Function):
    """raw_live [P',4] -> the 5-tuple of nerf_amd_volume_render_masked (alpha / w dense [B,N], zero at dead samples), with
    nerf_amd_volume_render_masked_backward.  ``head`` = (rays, jitter, tbins, flags, seed, ray_id0, mask, offsets)."""

    @staticmethod
    def forward(ctx, raw_live, head, B, N):
        rays, jit, tbins, flags, seed, ray_id0, mask, offsets = head
        dev = rays.device
        raw_live = raw_live.contiguous()
        rgb, disp, alpha, acc, w = _five_outputs(B, N, ALL_OUTPUTS, dev)
        _lib.launch("nerf_amd_volume_render_masked", raw_live if raw_live.numel() else None, rays, jit, tbins, flags, int(seed),
                    int(ray_id0), mask, offsets, rgb, disp, alpha, acc, w, B, N, dev=dev)
        ctx.save_for_backward(raw_live, rays, jit, tbins, mask, offsets)
        ctx.args = (flags, int(seed), int(ray_id0), B, N)
        if N == 1:        # the reference's empty sample axis (utils/rendering.py:60-61; csrc/composite_device.h)
            alpha, w = alpha[:, :0], w[:, :0]
        return rgb, disp, alpha, acc, w

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_alpha, g_acc, g_w):
        raw_live, rays, jit, tbins, mask, offsets = ctx.saved_tensors
        flags, seed, ray_id0, B, N = ctx.args
        dev = rays.device
        d_raw = torch.empty_like(raw_live)
        g_rgb, g_disp, g_alpha, g_acc, g_w = map(_grad_arg, (g_rgb, g_disp, g_alpha, g_acc, g_w))
        live = raw_live.numel() > 0
        _lib.launch("nerf_amd_volume_render_masked_backward", raw_live if live else None, rays, jit, tbins, flags, seed, ray_id0,
                    mask, offsets, g_rgb, g_disp, g_alpha, g_acc, g_w, d_raw if live else None, B, N, dev=dev)
        return d_raw, None, None, None


class _MaskedSigmaNoise(torch.autograd.Function):
    """raw_live [P',4] -> the same with sigma' = sigma + std z in column 3 (nerf_amd_sigma_noise_masked: the noise each live
    sample would get in the dense raw [B,N,4], keyed by its ORIGINAL index).  d sigma' / d sigma = 1: the backward is the
    identity.  ``head`` = (mask, offsets, B, N)."""

    @staticmethod
    def forward(ctx, raw_live, std, noise_seed, ray_id0, head):
        mask, offsets, B, N = head
        dev = raw_live.device
        raw_live = raw_live.contiguous()
        out = torch.empty_like(raw_live)
        live = raw_live.numel() > 0
        _lib.launch("nerf_amd_sigma_noise_masked", raw_live if live else None, out if live else None, float(std), 0,
                    int(noise_seed) & (2 ** 64 - 1), None, int(ray_id0), mask, offsets, B, N, dev=dev)
        return out

    @staticmethod
    def backward(ctx, g):
        return g, None, None, None, None


class _ZeroParamGrads(torch.autograd.Function):
    """An empty raw_live [0,4] that still hangs on the parameters: a batch with no live sample launches no network kernel
    and its backward hands every parameter a zero tensor, not None."""

    @staticmethod
    def forward(ctx, *params):
        ctx.like = params
        return torch.empty((0, 4), dtype=torch.float32, device=params[0].device)

    @staticmethod
    def backward(ctx, _g):
        return tuple(torch.zeros_like(p) for p in ctx.like)


def _masked_outputs(rays, net, N, occupancy, tbins, jit, flags, seed, ray_id0, mark=None, c=None):
    """The stages of ``render_nerf_masked`` once rays and jitter are settled: mark (or ``mark``, the ready MarkResult of these
    positions: the masked guided placement produces it with them) -> emit -> training forward on the live points -> masked
    compositor, with gradients.  Sets ``occupancy.last_stats``.
    ``c``: the ``Resolved`` controls or None: the noise stage on the live rows in front of the compositor, the blend behind it,
    and the sample positions attached to the weights as ``w.ts`` (``composite_with_controls``)."""
    from .utils import occupancy as occ_mod
    B = rays.size(0)
    m = occ_mod._mark(occupancy, rays, jit, tbins, flags, seed, ray_id0, N) if mark is None else mark
    pts = occ_mod._points(m, rays, jit, tbins, flags, seed, ray_id0)
    stats = {"rays": B, "samples": B * N, "live": m.live, "network_launches": 0}
    occupancy.last_stats = stats
    params = [p for _, p in net.named_parameters()]
    if m.live:
        # the reference's |x| > 1 warning, on the points the network is asked about (lazily, as Nerf.forward does)
        from .utils.xyz import range_check_values
        range_check_values(pts)
        raw_live, _ = _FusedDense.apply(net, None, None, None, 0, 0, 0, 1, pts, *params)
        raw_live = raw_live.reshape(-1, 4)
        stats["network_launches"] = 1
    else:
        raw_live = _ZeroParamGrads.apply(*params)
    positions = None if c is None else lambda: occ_mod.sample_positions(rays, jit, tbins, flags, seed, ray_id0, N)
    return composite_with_controls(raw_live, positions, None, None, c,
                                   masked=((rays, jit, tbins, flags, seed, ray_id0, m.mask, m.offsets), B, N))


def render_nerf_masked(rays, net, N, occupancy, tn=2, tf=6, *, u=None, ts=None, device_rng=False, seed=0, ray_id0=0,
                       return_ts=False, controls=None, box=None):
    """``render_nerf`` through an occupancy grid WITH gradients to the parameters of ``net``: the network is evaluated
    (fused bf16 training kernels, points mode) at the live samples only, a dead sample is (0, 0, 0, -inf) -- it contributes
    exactly nothing and receives no gradient.  Returns the same 5-tuple; alpha / w are dense [B,N], zero at dead samples.

    Stages: mark + scan -> ONE host read of the live count P' -> emit pts[P',6] -> training forward on the points ->
    masked compositor; backward: masked compositor backward -> dX chain -> dW products.  With P' = 0 no network kernel is
    launched and every parameter gradient is a zero tensor.  Sets ``occupancy.last_stats``.  Raises, before any jitter is
    drawn, for rays that require grad, precision='fp32' modules, other network sizes, foreign nets and N > 512.
    ``return_ts=True``: returns (5-tuple, ts [B,N]) -- the sample positions of this jitter as nerf_amd_query_points forms
    them (the coarse pass of the masked pair hands them to the sampler).
    ``controls``: a ``Controls`` -- Gaussian noise on the live rows of the raw density (nerf_amd_sigma_noise_masked: a live
    sample draws what the dense render gives that sample; a dead one stays dead) and rgb + (1 - acc) background behind the
    masked compositor; ``w.ts`` then holds the sample positions.  The distortion term belongs to the step: a non-zero
    ``controls.distortion`` raises ValueError.
    ``box``: a ``SceneBox`` or a ``GridSpan`` (utils/box.py) -- the samples are placed inside the box (``box.positions`` with this call's jitter
    arguments, formed once where the jitter would be drawn) and the call goes on as its ``ts=`` path; the positions carry no
    gradient.  Together with ``ts=``: ValueError."""
    from .utils.box import check_box
    check_box(box, ts=ts)
    controls = controls_mod.bundle(controls)
    if controls is not None and controls.distortion:
        raise ValueError("render_nerf_masked renders: the distortion term belongs to the step (train_step(..., occupancy=, "
                         "controls=), or distortion_loss on the weights it returns)")
    return _render_nerf_masked(rays, net, N, occupancy, tn, tf, controls, u=u, ts=ts, device_rng=device_rng, seed=seed,
                               ray_id0=ray_id0, return_ts=return_ts, box=box)


def _render_nerf_masked(rays, net, N, occupancy, tn, tf, c, *, u=None, ts=None, device_rng=False, seed=0, ray_id0=0,
                        return_ts=False, box=None):
    """The body of ``render_nerf_masked`` behind its preamble.  ``c``: a Controls, resolved here where the parent looked at the
    background's shape (behind the grid's checks, before the jitter is drawn), or a ``Resolved`` as a train step hands it down."""
    from .utils import box as box_mod, jitter, occupancy as occ_mod
    B, N = _lib.require_rays(rays), int(N)
    dev = rays.device
    occ_mod.check_trainable(occupancy, net, rays, N)
    if N < 1:
        raise RuntimeError(f"masked training serves 1 <= N <= {occ_mod.MAX_N_TRAIN} samples per ray, got N = {N}")
    _lib.require_same_device("occupancy grid", occupancy.words, dev)
    if isinstance(c, Controls):
        c = controls_mod.resolve(c, B, dev, ray_id0)       # the background's shape: before the jitter is drawn
    net.packed_weights(_lib.BF16)             # packs now if it has to: errors surface before the jitter is drawn
    if box is not None:                       # the box's positions, then the ts= path
        jitter.check(B, N, u=u)
        box_mod.check_interval(N, tn, tf)
        jit, flags, pending = box_mod.single(box, rays, N, tn, tf, u=u, device_rng=device_rng, seed=seed, ray_id0=ray_id0)
    else:
        jit, flags, pending = jitter.single(B, N, dev, u=u, ts=ts, device_rng=device_rng)
    try:
        rays = rays.detach().contiguous()
        tbins = jitter.tbins(tn, tf, N, dev, flags)
        out = _masked_outputs(rays, net, N, occupancy, tbins, jit, flags, seed, ray_id0, c=c)
        if return_ts:
            return out, occ_mod.sample_positions(rays, jit, tbins, flags, seed, ray_id0, N)
        return out
    finally:
        if pending is not None:
            pending.finish()


# --------------------------------------------------------------------------
# one optimisation step (reference train.py:47-57)
# --------------------------------------------------------------------------
def lr_decay_factor(lr_init, lr_final, num_iters):
    """Per-iteration multiplicative decay (reference train.py:36-39)."""
    import math
    return math.exp(math.log(lr_final / lr_init) / num_iters)


def _optimise(loss, params, optimizer, decay, group):
    """The tail of an eager optimisation step (train.py:53-57): backward, the gradients averaged over ``group``, the
    optimizer's step, the learning-rate decay.  Returns the detached loss."""
    from . import parallel
    loss.backward()
    parallel.allreduce_gradients(params, group=group)
    optimizer.step()
    if decay != 1.0:
        for pg in optimizer.param_groups:
            pg["lr"] = pg["lr"] * decay
    return loss.detach()


def _optimise_with_term(rgb, gt, w, ts, lam, tn, tf, params, optimizer, decay, group):
    """MSE(rgb, gt), with ``lam`` > 0 plus the distortion term on the weights ``w`` at ``ts`` (one fp32 add), through
    ``_optimise``; the detached total, ``.distortion`` on it the weighted term."""
    loss, term = mse_loss(rgb, gt), None
    if lam > 0:
        term = _distortion_term(w, ts, lam, tn, tf)
        loss = loss + term
    out = _optimise(loss, params, optimizer, decay, group)
    if term is not None:
        out.distortion = term.detach()
    return out


def train_step(net, optimizer, rays, gt, N, *, tn=2, tf=6, u=None, decay=1.0, group=None,
               precision=None, device_rng=False, seed=0, ray_id0=0, occupancy=None, background=None, sigma_noise=0.0,
               noise_seed=0, distortion=0.0, controls=None, box=None):
    """zero_grad -> render_nerf -> MSELoss(rgb, gt) -> backward -> [grad all-reduce]
    -> optimizer.step -> lr *= decay.  Returns the (detached) loss.
    Only ``rgb`` feeds the loss, as in the reference (train.py:52).
    The dense layers train in bf16 whatever the module's inference precision ('bf16' or 'fp16');
    precision 'fp32' trains exactly, layer by layer in fp32 (utils/generic_mlp.py): slow, and the reference's numbers.
    occupancy: an ``OccupancyGrid`` -- the render is ``render_nerf_masked`` (the network sees the live samples only; one
    host synchronisation per step); everything else is the same step.
    background, sigma_noise, noise_seed: ``render_nerf``'s -- the loss is MSELoss(rgb + (1 - acc) background, gt) and the raw
    density carries Gaussian noise of that standard deviation (counter RNG keyed by ``noise_seed``: pass a new one per step).
    Dense path only: with ``occupancy`` either raises RuntimeError before anything is drawn or launched.
    distortion: the weight lambda of mip-NeRF 360's distortion loss on the compositor's weights (0 = off, the default): the
    loss becomes MSE + lambda / (B (tf - tn)) sum_rays D (``distortion_loss``; one fp32 add), on every path that composites
    through the HIP backward (bf16 fused, precision='fp32', other sizes) and together with background / sigma_noise.  Dense
    path only (RuntimeError with ``occupancy``); negative or not finite: ValueError.  The returned loss is the total; with
    lambda > 0 ``.distortion`` on it holds the weighted term.
    controls: a ``Controls`` -- the same four as ONE argument, on the dense path (bit for bit the flat keywords; giving both
    raises ValueError) AND with ``occupancy``: the masked step with the noise on its live rows, the loss behind the background
    and the distortion term on the masked compositor's weights, assembled as the dense step assembles them.
    box: a ``SceneBox`` or a ``GridSpan`` (utils/box.py; DESIGN.md sections 33 and 39) -- the samples are placed inside the box: the step is this step on
    ``render_nerf(..., box=box)`` / ``render_nerf_masked(..., box=box)``, dense or with ``occupancy``, with the controls, at
    every precision.  The positions carry no gradient; the distortion term keeps the global ``tf`` and its coefficient."""
    from .utils.box import check_box
    bkw = {} if check_box(box) is None else {"box": box}       # off by default: a call without it is the call it was
    c = controls_mod.from_keywords(controls, {"occupancy": occupancy}, background=background, sigma_noise=sigma_noise,
                                   noise_seed=noise_seed, distortion=distortion)
    if occupancy is not None:
        from .utils.occupancy import check_trainable
        check_trainable(occupancy, net, rays, N, precision)      # before zero_grad: a refused call changes nothing
    if c is not None:
        c = controls_mod.resolve(c, _lib.require_rays(rays), rays.device, ray_id0)     # the background's shape, likewise
    optimizer.zero_grad(set_to_none=True)
    if occupancy is not None:
        rgb, _, _, _, w = _render_nerf_masked(rays, net, N, occupancy, tn, tf, c, u=u, device_rng=device_rng, seed=seed,
                                              ray_id0=ray_id0, **bkw)
    else:
        rgb, _, _, _, w = _render_nerf(rays, net, N, tn, tf, c, u=u, precision=precision, device_rng=device_rng, seed=seed,
                                       ray_id0=ray_id0, **bkw)
    return _optimise_with_term(rgb, gt, w, getattr(w, "ts", None), 0.0 if c is None else c.lam, tn, tf, net.parameters(), optimizer,
                               decay, group)


# --------------------------------------------------------------------------
# the hierarchical pair (BASELINE config 4): coarse and fine networks trained together
# --------------------------------------------------------------------------
def _check_pair(net_c, net_f, Nc, Nf, precision):
    """The pair's limits, checked before anything is drawn or launched: two distinct modules with one precision, and
    nerf_amd_sample_pdf's sample counts (3 <= Nc <= 256, 0 <= Nf, Nc + Nf <= 512)."""
    if net_c is net_f:
        raise ValueError("the coarse and the fine network must be two distinct modules")
    if net_c.precision != net_f.precision:
        raise ValueError(f"the coarse and the fine network differ in precision ({net_c.precision!r} vs {net_f.precision!r})")
    _lib.require_pair_sizes(int(Nc), int(Nf))
    return _lib.precision_of(net_c, precision)


def _pair_stats(coarse, fine):
    """``occupancy.last_stats`` of a masked pair render: the sums, and each pass's own report."""
    out = {k: coarse[k] + fine[k] for k in ("samples", "live", "network_launches")}
    out.update(rays=coarse["rays"], coarse=coarse, fine=fine)
    return out


def _render_train_with_ts(rays, net, N, tn, tf, jit, flags, precision, seed, ray_id0, c=None):
    """render_nerf_autograd that also hands back the sample positions it drew (the coarse pass of the pair).
    ``c``: the ``Resolved`` controls of ``composite_with_controls``; None = none, and ``w.ts`` is not set."""
    from .utils.xyz import range_check_rays
    dev, B = rays.device, rays.size(0)
    tbins = _tbins(tn, tf, N, dev)
    range_check_rays(rays, jit, tbins, flags, seed, ray_id0, N)
    if _lib.precision_code(precision) == _lib.F32:
        from .utils import generic_mlp
        q = torch.empty((B * N, 6), dtype=torch.float32, device=dev)
        ts = torch.empty((B, N), dtype=torch.float32, device=dev)
        _lib.launch("nerf_amd_query_points", rays, jit, tbins, flags, int(seed), int(ray_id0), q, ts, B, N, dev=dev)
        raw = generic_mlp.forward(net, q).reshape(B, N, 4).float()
    else:
        params = [p for _, p in net.named_parameters()]
        raw, ts = _FusedDense.apply(net, rays, jit, tbins, flags, seed, ray_id0, N, None, *params)
    if c is not None:
        return composite_with_controls(raw, ts, rays, True, c), ts
    return _VolumeRender.apply(raw, ts, rays, True), ts


def train_step_hierarchical(net_c, net_f, optimizer, rays, gt, Nc=64, Nf=128, *, tn=2, tf=6, u_c=None, u_f=None,
                            decay=1.0, group=None, precision=None, device_rng=False, seed=0, ray_id0=0, occupancy=None,
                            controls=None, box=None):
    """One optimisation step of the coarse / fine pair (the NeRF paper's objective; the reference has no hierarchical
    path, its CoarseNet / FineNet are empty): zero_grad -> coarse render_nerf with gradients (Nc stratified samples) ->
    sample_pdf on the DETACHED coarse weights (the coarse net learns from its own loss only) -> fine render_nerf of
    ``net_f`` on the Nc+Nf merged positions with gradients -> MSE(rgb_c, gt) + MSE(rgb_f, gt) -> backward ->
    [all-reduce of the combined gradient, one bucket] -> optimizer.step -> lr *= decay.

    ``optimizer``: ``optim.FusedAdam([net_c, net_f])`` or any torch optimizer over exactly both modules' parameters.
    Jitter: ``u_c`` [B,Nc] / ``u_f`` [B,Nf]; default the render_hierarchical draws, torch.rand(B,Nc) then
    torch.rand(B,Nf) from torch's CPU generator (continued on the device); ``device_rng=True``: the counter RNG keyed by
    (seed, ray_id0 + ray).  precision 'fp32' trains both exactly, layer by layer (utils/generic_mlp.py).
    Returns the detached total loss; ``.losses`` on it holds the [coarse, fine] terms, ``.ts_f`` the fine positions.

    occupancy: ONE ``OccupancyGrid`` masks both passes: the coarse pass is ``render_nerf_masked``
    on the Nc stratified samples, the sampler sees its weights (exactly 0 at a dead sample; a ray with no live coarse
    sample gets uniform fine samples), the fine pass is ``render_nerf_masked(ts=ts_f)`` through the same grid.  Two host
    synchronisations per step (one live count per pass); ``occupancy.last_stats`` holds the sums and the two passes'
    own reports under 'coarse' / 'fine'.  The default network and the bf16 training kernels only, rays without
    requires_grad; refused before any jitter is drawn.

    controls: a ``Controls`` with a background and / or sigma noise, dense or with ``occupancy``: the
    loss is MSE(rgb_c + (1 - acc_c) bg, gt) + MSE(rgb_f + (1 - acc_f) bg, gt) and both passes carry Gaussian noise of
    ``controls.sigma_noise`` on the raw density -- the coarse pass keyed by ``noise_seed``, the fine pass by ``noise_seed +
    FINE_NOISE_OFFSET`` (mod 2^64), both with this call's ``ray_id0``.  The sampler sees the (detached) weights of the noisy
    coarse compositor; the background never touches them.  ``controls.distortion > 0`` raises RuntimeError before anything
    else is looked at: the term belongs on the final weights, not on what places the samples."""
    from .optim import FusedAdam
    from .utils import jitter
    from .utils.box import refuse_box
    c = controls_mod.pair(controls, "train_step_hierarchical")
    refuse_box(box, "the coarse + fine pair (train_step_hierarchical)")
    _check_pair(net_c, net_f, Nc, Nf, precision)
    Nc, Nf = int(Nc), int(Nf)
    params = list(net_c.parameters()) + list(net_f.parameters())
    if isinstance(optimizer, FusedAdam):
        if optimizer.nets is None or len(optimizer.nets) != 2 or optimizer.nets[0] is not net_c or optimizer.nets[1] is not net_f:
            raise RuntimeError("the optimizer is not FusedAdam([net_c, net_f]) of this pair")
    else:
        opt_ids = {id(p) for pg in optimizer.param_groups for p in pg["params"]}
        if opt_ids != {id(p) for p in params}:
            raise RuntimeError("the optimizer does not hold exactly the parameters of the coarse and the fine network")
    B, dev = _lib.require_rays(rays), rays.device
    _lib.require_shape(u_c, "u_c", (B, Nc))
    _lib.require_shape(u_f, "u_f", (B, Nf))
    if occupancy is not None:
        from .utils.occupancy import check_trainable
        check_trainable(occupancy, net_c, rays, Nc, precision)       # before any draw: a refused call changes nothing
        check_trainable(occupancy, net_f, rays, Nc + Nf, precision)
        _lib.require_same_device("occupancy grid", occupancy.words, dev)
    c = controls_mod.resolve(c, B, dev, ray_id0)        # the background's shape: before any draw
    # off by default: a call without controls is the call it was, the fine pass's default ray_id0 included
    c_f, kw_f = (None, {}) if c is None else (c.fine(), {"ray_id0": ray_id0})
    rays = rays.detach().contiguous()
    jit_c, flags, u_f = jitter.pair(B, Nc, Nf, dev, u_c=u_c, u_f=u_f, device_rng=device_rng)

    optimizer.zero_grad(set_to_none=True)
    if occupancy is not None:
        coarse, ts_c = _render_nerf_masked(rays, net_c, Nc, occupancy, tn, tf, c, u=jit_c, device_rng=jit_c is None, seed=seed,
                                           ray_id0=ray_id0, return_ts=True)
        stats_c = occupancy.last_stats
    else:
        coarse, ts_c = _render_train_with_ts(rays, net_c, Nc, tn, tf, jit_c, flags,
                                             net_c.precision if precision is None else precision, seed, ray_id0, c)
    # the fine positions carry no gradient: w.detach() -- the coarse net learns from MSE(rgb_c, gt) alone.  With sigma noise
    # these are the weights of the noisy compositor; a background never touches them
    ts_f = sample_pdf(ts_c, coarse[4].detach(), Nf, u=u_f, device_rng=device_rng, seed=seed, ray_id0=ray_id0)
    if occupancy is not None:
        fine = _render_nerf_masked(rays, net_f, Nc + Nf, occupancy, tn, tf, c_f, ts=ts_f, **kw_f)
        occupancy.last_stats = _pair_stats(stats_c, occupancy.last_stats)
    else:
        fine = _render_nerf(rays, net_f, Nc + Nf, tn, tf, c_f, ts=ts_f, precision=precision, **kw_f)
    loss_c = mse_loss(coarse[0], gt)
    loss_f = mse_loss(fine[0], gt)
    loss = loss_c + loss_f
    out = _optimise(loss, params, optimizer, decay, group)
    out.losses, out.ts_f = [loss_c.detach(), loss_f.detach()], ts_f
    return out


# --------------------------------------------------------------------------
# grid-guided fine sampling: ONE network, its Nf new samples placed from a sigma volume
# --------------------------------------------------------------------------
def train_step_guided(net, optimizer, rays, gt, Nc, Nf, proposal, *, tn=2, tf=6, u_c=None, ts_c=None, u_f=None, decay=1.0,
                      group=None, precision=None, device_rng=False, seed=0, ray_id0=0, occupancy=None, distortion=0.0,
                      controls=None, box=None):
    """One optimisation step of ONE network on grid-guided positions: ts = ``proposal.sample(rays, Nc, Nf, ...)`` (a
    ``ProposalVolume``, utils/proposal.py: no network evaluation, no gradient) -> zero_grad -> render_nerf with gradients on those
    Nc + Nf positions -> MSE(rgb, gt) -> backward -> [grad all-reduce] -> optimizer.step -> lr *= decay.  The loss is that of
    the existing eager step on the same explicit ``ts``, bit for bit; nothing of ``proposal`` receives a gradient.
    Jitter as ``ProposalVolume.sample`` (default: render_hierarchical's draws, torch.rand(B,Nc) then torch.rand(B,Nf) from
    torch's CPU generator).  Refreshing the volume (``proposal.update(net)``) is the caller's schedule.
    Returns the detached loss; ``.ts`` on it holds the positions.

    occupancy: an ``OccupancyGrid`` -- the masked guided step: the masked guided placement (dead coarse
    samples weigh nothing; the merged positions come back marked, one host read) -> the stages of ``render_nerf_masked`` on
    those positions under that mark, which is not formed again.  The loss is that of ``render_nerf_masked(rays, net, Nc + Nf,
    occupancy, ts=ts)``, bit for bit; refused as that function refuses (precision='fp32', other network sizes, foreign nets),
    before anything is drawn.

    distortion: ``train_step``'s -- the loss becomes MSE + lambda / (B (tf - tn)) sum_rays D on the Nc + Nf guided positions.
    Not with ``occupancy`` (RuntimeError before anything is drawn).

    controls: a ``Controls`` -- with ``occupancy`` the masked guided step with the three terms, as ``train_step(..., occupancy=,
    controls=)`` on the guided positions (the noise is keyed by ``noise_seed`` and ``ray_id0``).  Without a grid it stands for
    ``distortion`` alone (the dense guided step knows no background and no noise: RuntimeError); with the flat keyword:
    ValueError.
    box: refused (RuntimeError before anything is drawn): the guided placement has its own interval."""
    from .utils.box import refuse_box
    refuse_box(box, "the guided step (train_step_guided)")
    c = controls_mod.from_keywords(controls, {"occupancy": occupancy}, distortion=distortion)
    if controls is not None and occupancy is None and (c.background is not None or c.sigma_noise):
        raise RuntimeError("the dense guided step takes the distortion term only: background / sigma_noise need occupancy=")
    lam = 0.0 if c is None else c.distortion
    _check_guided(net, proposal)
    _lib.precision_of(net, precision)             # a precision the kernels do not know: ValueError before anything else
    if occupancy is not None:
        from .utils import occupancy as occ_mod
        occ_mod.check_trainable(occupancy, net, rays, int(Nc) + int(Nf), precision)
    proposal.check(rays, Nc, Nf, u_c, ts_c, u_f, device_rng, occupancy=occupancy)   # before any draw: a refused call changes nothing
    if occupancy is not None:
        c = controls_mod.resolve(c, rays.size(0), rays.device, ray_id0)        # the background's shape: before any draw
        net.packed_weights(_lib.BF16)             # packs now if it has to: errors surface before the jitter is drawn
        rays = rays.detach().contiguous()
        ts, mark = proposal.sample(rays, Nc, Nf, tn, tf, u_c=u_c, ts_c=ts_c, u_f=u_f, device_rng=device_rng, seed=seed,
                                   ray_id0=ray_id0, occupancy=occupancy, return_mark=True)
        optimizer.zero_grad(set_to_none=True)
        outs = _masked_outputs(rays, net, int(Nc) + int(Nf), occupancy, None, ts, _lib.FLAG_TS_GIVEN, 0, 0, mark=mark, c=c)
    else:
        ts = proposal.sample(rays, Nc, Nf, tn, tf, u_c=u_c, ts_c=ts_c, u_f=u_f, device_rng=device_rng, seed=seed,
                             ray_id0=ray_id0)
        rays = rays.detach().contiguous()
        optimizer.zero_grad(set_to_none=True)
        outs, _ = _render_train_with_ts(rays, net, int(Nc) + int(Nf), tn, tf, ts, _lib.FLAG_TS_GIVEN,
                                        net.precision if precision is None else precision, seed, ray_id0)
    out = _optimise_with_term(outs[0], gt, outs[4], ts, lam, tn, tf, net.parameters(), optimizer, decay, group)
    out.ts = ts
    return out


# --------------------------------------------------------------------------
# the same step as ONE captured hipGraph (launch-bound at 4096-ray batches)
# --------------------------------------------------------------------------
class _HyperRing:
    """Pinned host ring for the per-step scalars (Adam's six floats + the jitter seed offset as an int64): one slot per
    step, written by the host before it launches the step and read on the device by the first node of graph A
    (nerf_amd_hyper_fetch: slot = device counter % slots) -- no copy between two graph launches.  A slot is rewritten only
    after the event recorded behind the launch that read it has completed.

    Lockstep: the host index ``k`` must name the slot the device counter names.  ``push`` opens a
    step (``pending``) and ``launched`` closes it; a ``push`` that finds the previous step still open -- an exception or a
    KeyboardInterrupt between the two, with the replay enqueued or not: the host cannot know -- takes ``k`` from the device
    counter itself (one wait for the stream, on that path only), so the slot it writes is the one the next replay reads.
    ``reset`` puts both back to 0."""

    def __init__(self, dev, slots=16):
        self.ring = torch.zeros((slots, 8), dtype=torch.float32).pin_memory()
        with torch.cuda.device(dev):
            self.ring_dev = int(_lib.lib().nerf_amd_pinned_device_address(_lib.ptr(self.ring)))
        if self.ring_dev <= 0:
            raise RuntimeError("the pinned host ring of the step's scalars is not mapped into the device's address space")
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.events = [None] * slots
        self.k, self.pending = 0, False

    def reset(self):
        self.k, self.pending = 0, False
        self.counter.zero_()

    def _resync(self):
        """The step before this one never reached ``launched``: the device counter says how many replays were enqueued.
        Reading it waits for all of them, so no slot is in flight any more."""
        torch.cuda.synchronize(self.counter.device)
        self.k = int(self.counter.item()) & 0xffffffff
        self.events = [None] * len(self.events)

    def push(self, values, seed_offset=0):
        if self.pending:
            self._resync()
        self.pending = True
        i = self.k % self.ring.shape[0]
        if self.events[i] is not None:
            self.events[i].synchronize()
            self.events[i] = None
        h = self.ring[i]
        for j, v in enumerate(values):
            h[j] = v
        h[6:8].view(torch.int64)[0] = int(seed_offset)

    def fetch(self, dst, dev):
        """Enqueue (or capture) the device-side read of the next slot into ``dst``."""
        _launch("nerf_amd_hyper_fetch", self.ring_dev, int(self.ring.shape[0]), dst, self.counter, _lib.stream_ptr(dev))

    def launched(self, dev):
        """The launch that reads the slot just pushed is in the stream."""
        i = self.k % self.ring.shape[0]
        self.k = (self.k + 1) & 0xffffffff                      # the device counter is 32 bits wide and wraps with it
        self.pending = False
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self.events[i] = ev


class _StatusWatch:
    """Asynchronous read-back of the status words behind a packed 16-bit weight image (include/nerf_amd.h
    nerf_amd_packed_status_offset): the training forward sets word 0 when a point shows a non-finite value inside the
    network, the re-pack of every step sets word 1 when a weight is not finite.  In the reference such a step ends in a NaN loss for everyone to see; here the kernels' integer ReLU can
    turn the NaNs into finite garbage, so the flag is what makes a diverged run loud.  ``push`` enqueues an 8-byte copy
    into pinned memory behind the forward, ``poll`` looks at the copies that have completed -- no host wait."""

    def __init__(self, slots=4):
        self.bufs = [torch.zeros(2, dtype=torch.int32).pin_memory() for _ in range(slots)]
        self.pending = []                       # (event, slot, step)
        self.k = 0

    def push(self, packed, step):
        if len(self.pending) >= len(self.bufs):
            return                              # every slot still in flight: skip this sample
        slot = self.k % len(self.bufs)
        self.k += 1
        off = int(_lib.lib().nerf_amd_packed_status_offset(_lib.BF16))
        self.bufs[slot].copy_(packed[off:off + 8].view(torch.int32), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(packed.device))
        self.pending.append((ev, slot, step))

    def poll(self):
        """The first completed sample with a flag set, as (step, activations flagged, weights flagged), or None."""
        hit = None
        while self.pending and self.pending[0][0].query():
            _, slot, step = self.pending.pop(0)
            words = (int(self.bufs[slot][0]), int(self.bufs[slot][1]))
            if hit is None and (words[0] != 0 or words[1] != 0):
                hit = (step, words[0] != 0, words[1] != 0)
        return hit

    def raise_if_diverged(self, unit):
        """FloatingPointError once a completed sample shows a flag; ``unit`` names what the sample's number counts."""
        bad = self.poll()
        if bad is not None:
            what = " and ".join(w for w, on in (("activations", bad[1]), ("weights", bad[2])) if on)
            raise FloatingPointError(f"non-finite values inside the network in training {unit} {bad[0]} ({what}): "
                                     "NaN / inf weights or inputs, the run has diverged")


class _CountsWatch:
    """Asynchronous read-back of the graphed masked step's ``counts`` (int64[2] = {live, kept}), after _StatusWatch: ``push``
    enqueues a 16-byte copy into pinned memory behind graph A, ``poll`` hands back the copies that have completed, oldest
    first, as (step, live, kept) -- no host wait."""

    def __init__(self, slots=4, width=2):
        self.bufs = [torch.zeros(width, dtype=torch.int64).pin_memory() for _ in range(slots)]
        self.pending = []                       # (event, slot, step)
        self.k = 0

    def push(self, counts, step):
        if len(self.pending) >= len(self.bufs):
            return                              # every slot still in flight: skip this sample
        slot = self.k % len(self.bufs)
        self.k += 1
        self.bufs[slot].copy_(counts, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(counts.device))
        self.pending.append((ev, slot, step))

    def poll(self, wait=False):
        done = []
        while self.pending and (wait or self.pending[0][0].query()):
            ev, slot, step = self.pending.pop(0)
            if wait:
                ev.synchronize()
            done.append((step, *(int(v) for v in self.bufs[slot])))
        return done


class _GuardWatch(_CountsWatch):
    """Asynchronous read-back of a guarded optimiser's record (``FusedAdam(max_grad_norm=)``: eight 32-bit words), after
    _CountsWatch: ``push`` enqueues the 32-byte copy into pinned memory behind graph B, ``risen`` hands back, for each
    completed copy whose skipped counter stands above the last one seen, (step, steps withheld since) -- no host wait."""

    def __init__(self, slots=4):
        self.bufs = [torch.zeros(8, dtype=torch.int32).pin_memory() for _ in range(slots)]
        self.pending, self.k, self.skipped = [], 0, 0

    def push(self, guard, step):
        super().push(guard.view(torch.int32), step)

    def risen(self):
        out = []
        for step, *words in self.poll():
            if words[5] > self.skipped:
                out.append((step, words[5] - self.skipped))
                self.skipped = words[5]
        return out


def _capacity_points(capacity, total, what):
    """A capacity argument as points: an int is a number of points, a float a fraction of ``total`` (GraphedMaskedTrainStep's
    rule).  ``what`` names the argument in the messages."""
    import math
    import numbers
    if isinstance(capacity, bool) or not isinstance(capacity, numbers.Real):
        raise TypeError(f"{what} must be an int (points) or a float (fraction of the pass's samples)")
    if isinstance(capacity, numbers.Integral):
        C = int(capacity)
    else:
        if not 0.0 < capacity <= 1.0:
            raise ValueError(f"a fractional {what} must lie in (0, 1], got {capacity!r}")
        C = max(1, math.ceil(float(capacity) * total))
    if not 1 <= C <= total:
        raise ValueError(f"{what} must lie in [1, {total}] points, got {C}")
    return C


def _launch(name, *args):
    """``_lib.launch`` as the captured sequences spell it: the stream is the last argument.  The steppers reach it through
    this module global (a test counts the launches of a capture here)."""
    _lib.launch(name, *args[:-1], stream=args[-1])


class _Pass:
    """What ONE network pass of a graphed step owns, and how each of its stages is enqueued.
    ``N`` samples per ray, network kernels on ``P`` points (``rows`` = the leading shape of raw / d_raw).  The stepper hands
    it the rest before the first launch: ``net`` and its images ``fwd`` / ``bwd``, ``grads`` (its slice of the flat gradient
    vector), ``loss`` (its loss slot) and ``jitter`` = (rays, jitter, tbins, flags, seed, ray_id0) as the kernels take them."""

    noise_offset = 0             # what this pass adds to the stepper's noise_seed (the fine pass of a pair: FINE_NOISE_OFFSET)

    def noise_seed(self):
        """The seed argument of this pass's sigma noise (the step's offset in memory comes on top)."""
        return (self.step.noise_seed + self.noise_offset) & (2 ** 64 - 1)

    def __init__(self, step, N, P, rows, e4m3=False):
        lib, dev = _lib.lib(), step.dev
        f32, u8 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.uint8, device=dev)
        self.step, self.N, self.P, self.e4m3 = step, N, P, e4m3
        self.raw, self.d_raw = torch.empty((*rows, 4), **f32), torch.empty((*rows, 4), **f32)
        self.rgb = torch.empty((step.B, 3), **f32)
        if e4m3:
            self.acts = torch.empty(int(lib.nerf_amd_train_activation_bytes_e4m3(P)), **u8)
            self.dys = torch.empty(int(lib.nerf_amd_train_gradient_bytes_e4m3(P)), **u8)
            self.scratch8 = torch.empty(max(int(lib.nerf_amd_param_gradients_scratch_e4m3_bytes(P)), 16), **u8)
        else:
            nb = int(lib.nerf_amd_train_activation_bytes(P))
            self.acts, self.dys = torch.empty(nb, **u8), torch.empty(nb, **u8)
        self.posx = torch.empty((P, 64), dtype=torch.bfloat16, device=dev)
        self.posd = torch.empty((P, 32), dtype=torch.bfloat16, device=dev)
        self.scratch = torch.empty(max(int(lib.nerf_amd_param_gradients_scratch_bytes(P)), 16), **u8)

    def dx_chain(self, st):
        _launch("nerf_amd_mlp_backward_e4m3" if self.e4m3 else "nerf_amd_mlp_backward",
                self.d_raw, self.bwd, self.acts, self.dys, self.P, st)

    def loss_and_begin(self, ss):
        """The loss value, then the gradient slice's zero fill and the d_raw pack."""
        _launch("nerf_amd_mse_loss", self.rgb, self.step.gt, self.loss, None, self.step.B * 3, ss)
        _launch("nerf_amd_param_gradients_begin", self.d_raw, self.scratch, self.grads, self.P, ss)
        if self.e4m3:        # the packed d_raw in the products' 8-bit form
            _launch("nerf_amd_param_gradients_convert_e4m3", None, None, self.scratch, self.scratch8, self.P, 2, ss)

    def finish(self, bucket, st):
        """The dW products (all, or one bucket's) from the saved tensors in this pass's storage form."""
        if self.e4m3:
            _launch("nerf_amd_param_gradients_finish_e4m3", self.acts, self.dys, self.scratch8, self.grads, self.P, bucket, st)
        else:
            _launch("nerf_amd_param_gradients_finish_bucket", self.acts, self.dys, self.posx, self.posd, self.scratch,
                    self.grads, self.P, bucket, st)


class _DensePass(_Pass):
    """All B x N samples: the forward samples the rays itself and writes the positions ``ts``."""

    def __init__(self, step, N, e4m3=False):
        super().__init__(step, N, step.B * N, (step.B, N), e4m3)
        self.ts = torch.empty((step.B, N), dtype=torch.float32, device=step.dev)

    def forward(self, st):
        rays, jit, tbins, flags, seed, rid = self.jitter
        _launch("nerf_amd_mlp_forward_train", rays, jit, tbins, self.fwd, flags | (_lib.FLAG_STORE_E4M3 if self.e4m3 else 0),
                seed, rid, self.raw, self.ts, self.acts, self.step.B, self.N, st)

    def head(self, st, pdf=None):
        """Compositor + MSE gradient + compositor backward, one kernel; only rgb feeds the loss (train.py:52): disparity,
        alpha, acc, w are not materialised.  ``pdf`` = (u_f, ts_f, Nf): sample_pdf on the weights in the same kernel (they
        never reach HBM), which takes the seed in memory where the counter RNG leaves u_f empty."""
        s, (rays, jit, _, flags, seed, rid) = self.step, self.jitter
        if pdf is None and s._distortion > 0:
            # the head with the distortion term beside the MSE (and behind the same controls, if any): still one launch; the
            # per-ray loss values go to the side branch's sum
            _launch("nerf_amd_volume_render_mse_backward_dist", self.raw, self.ts, rays, s.gt, s.background,
                    s._bg_stride, s.sigma_noise, _lib.FLAG_SEED_IN_MEMORY, self.noise_seed(), s._seed_mem, s.ray_id0,
                    s._t_far, s._dist_coef, self.rgb, s._loss_ray, self.d_raw, s.B, self.N, st)
        elif pdf is None and s._controls:
            # the same head behind the stepper's background and / or with noise on sigma; the noise key is noise_seed + the
            # step's offset in memory, whatever the jitter source is
            _launch("nerf_amd_volume_render_mse_backward_bg", self.raw, self.ts, rays, s.gt, s.background,
                    s._bg_stride, s.sigma_noise, _lib.FLAG_SEED_IN_MEMORY, self.noise_seed(), s._seed_mem, s.ray_id0,
                    self.rgb, self.d_raw, s.B, self.N, st)
        elif pdf is None:
            _launch("nerf_amd_volume_render_mse_backward", self.raw, self.ts, rays, s.gt, self.rgb, self.d_raw, s.B, self.N, st)
        elif s._controls:
            # the coarse head of a pair behind the stepper's background and / or with noise on sigma: the sampler sees the
            # weights of the noisy compositor.  The sampler and the noise share the stepper's ray_id0 (the sampler reads it with
            # the counter RNG only, where it is the jitter's own)
            u_f, ts_f, Nf = pdf
            _launch("nerf_amd_volume_render_mse_backward_pdf_bg", self.raw, self.ts, rays, s.gt, s.background, s._bg_stride,
                    s.sigma_noise, _lib.FLAG_SEED_IN_MEMORY, self.noise_seed(), s._seed_mem, jit if u_f is None else u_f,
                    flags, seed, s.ray_id0, self.rgb, self.d_raw, ts_f, s.B, self.N, Nf, st)
        else:
            u_f, ts_f, Nf = pdf
            _launch("nerf_amd_volume_render_mse_backward_pdf", self.raw, self.ts, rays, s.gt,
                    jit if u_f is None else u_f, flags, seed, rid, self.rgb, self.d_raw, ts_f, s.B, self.N, Nf, st)

    def encoder_rows(self, ss):
        """At the sample positions the forward drew: ts = f(jitter) bit for bit (the same jitter arguments)."""
        _launch("nerf_amd_sample_encode_bf16", *self.jitter, self.posx, self.posd, None, self.step.B, self.N, ss)
        if self.e4m3:        # the encoder rows in the products' 8-bit form
            _launch("nerf_amd_param_gradients_convert_e4m3", self.posx, self.posd, None, self.scratch8, self.P, 1, ss)


class _MaskedPass(_Pass):
    """The live samples of the stepper's occupancy grid, on a fixed capacity of P = C points: mark + scan, capped emit of
    ``pts`` [C, 6] (``counts`` = {live, kept}), then the points-mode kernels; rows no live sample owns are inert."""

    def __init__(self, step, N, C, counts):
        super().__init__(step, N, C, (C,))
        B, dev = step.B, step.dev
        self.mask = torch.zeros((B, (N + 63) // 64), dtype=torch.int64, device=dev)
        self.offsets = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        self.pts, self.counts = torch.empty((C, 6), dtype=torch.float32, device=dev), counts

    def forward(self, st):
        s, (*head, flags, seed, rid) = self.step, self.jitter
        R, lo, inv, outside = s._grid
        _launch("nerf_amd_occupancy_mark", *head, flags | outside, seed, rid, s._words_ptr, *R, lo, inv,
                self.mask, self.offsets, None, s._mark_ws, s.B, self.N, st)
        _launch("nerf_amd_occupancy_points_capped", *self.jitter, self.mask, self.offsets, self.pts, self.counts, self.P, s.B,
                self.N, st)
        _launch("nerf_amd_mlp_forward_train_points", self.pts, self.fwd, self.raw, self.acts, self.P, st)

    def head(self, st, pdf=None):
        """The masked head (masked compositor + MSE gradient + backward, one kernel); ``pdf`` as the dense pass's."""
        s = self.step
        args = (self.raw, *self.jitter, self.mask, self.offsets, s.gt)
        if pdf is None and (s._controls or s._distortion > 0):
            # the masked head behind the stepper's background, with noise on the live rows and / or with the distortion term
            # beside the MSE: still one launch.  The noise key is noise_seed + the step's offset in memory and its ray ids start
            # at the stepper's ray_id0, whatever the jitter source is (given positions carry no ids of their own)
            rays, jit, tbins, flags, seed, _ = self.jitter
            _launch("nerf_amd_volume_render_masked_mse_backward_dist", self.raw, rays, jit, tbins, flags, seed, s.ray_id0,
                    self.mask, self.offsets, s.gt, s.background, s._bg_stride, s.sigma_noise,
                    _lib.FLAG_SEED_IN_MEMORY, self.noise_seed(), s._seed_mem, s._t_far if s._distortion > 0 else 0.0,
                    s._dist_coef if s._distortion > 0 else 0.0, self.rgb, s._loss_ray if s._distortion > 0 else None,
                    self.d_raw, self.P, s.B, self.N, st)
        elif pdf is None:
            _launch("nerf_amd_volume_render_masked_mse_backward", *args, self.rgb, self.d_raw, self.P, s.B, self.N, st)
        elif s._controls:
            # the masked coarse head of a pair behind the stepper's background and / or with noise on the live rows: the
            # sampler sees the weights of the noisy masked compositor under the clamp; ray ids as in the branch above
            u_f, ts_f, Nf = pdf
            rays, jit, tbins, flags, seed, _ = self.jitter
            _launch("nerf_amd_volume_render_masked_mse_backward_pdf_bg", self.raw, rays, jit, tbins, flags, seed, s.ray_id0,
                    self.mask, self.offsets, s.gt, s.background, s._bg_stride, s.sigma_noise, _lib.FLAG_SEED_IN_MEMORY,
                    self.noise_seed(), s._seed_mem, u_f, self.rgb, self.d_raw, ts_f, self.P, s.B, self.N, Nf, st)
        else:
            u_f, ts_f, Nf = pdf
            _launch("nerf_amd_volume_render_masked_mse_backward_pdf", *args, u_f, self.rgb, self.d_raw, ts_f,
                    self.P, s.B, self.N, Nf, st)

    def encoder_rows(self, ss):
        _launch("nerf_amd_encode_points_bf16", self.pts, self.posx, self.posd, self.P, ss)


class _MarkedPass(_MaskedPass):
    """A masked pass whose ``mask`` / ``offsets`` the stepper's own launch in front of it has written (the masked guided
    placement, which marks the positions it places): capped emit, then the points-mode kernels -- no mark of its own."""

    def forward(self, st):
        _launch("nerf_amd_occupancy_points_capped", *self.jitter, self.mask, self.offsets, self.pts, self.counts, self.P,
                self.step.B, self.N, st)
        _launch("nerf_amd_mlp_forward_train_points", self.pts, self.fwd, self.raw, self.acts, self.P, st)


class GraphedTrainStep:
    """``train_step`` (reference train.py:47-57) for the fused bf16 path with every buffer
    allocated once and the launches captured into hipGraphs that are replayed per iteration:

        graph A: forward (saving activations) -> compositor + MSE gradient + compositor backward (one
                 kernel) -> dX chain -> all 24 parameter gradients, with the encoder rows, the loss
                 value, the gradient zero fill and the d_raw pack on a parallel branch
                 (9 kernel nodes, all through the C ABI: no torch kernels, no memset node)
        graph B: Adam over the flat parameter vector -> re-pack the two MFMA weight images (one kernel)

    This class holds the ONE launch sequence of graph A (``_forward_backward``) over ``passes``, the
    network passes of an iteration; its subclasses choose the passes -- one or two (coarse and fine), each dense (B x N
    samples) or masked (the live samples of an occupancy grid on a fixed capacity) -- and add their own bookkeeping.

    With a process group of more than one replica the flat gradient vector is averaged between graph A and graph B:

        buckets=1 (default)  ONE in-place all-reduce of the 2.38 MB vector; fully exposed, and the cheapest form
                             measured: +16 ... 26 us per step with RCCL on one rank (1.185 -> 1.201 ms).
        buckets=2            the gradients are produced in two launches and reduced in two buckets
                             (include/nerf_amd.h nerf_amd_grad_bucket_range):
                               graph A1: ... -> dX chain -> gradients of the LATE layers (the tail of the vector)
                               all-reduce of that bucket (1.27 MB) starts on the collective's own stream
                               graph A2: gradients of layers_0.* (the head)      <- runs while bucket 1 is on the wire
                               all-reduce of the head bucket (1.12 MB); both awaited; graph B
                             Only the second exchange is exposed -- but the split itself costs 75 ... 90 us per step (a
                             second 64 MB tail of split-K atomics and a second ramp of the HBM-bound gradient kernel),
                             measured with RCCL on one rank: 1.288 vs 1.201 ms.  It pays only where one 1.27 MB
                             all-reduce takes longer than that.

    ``timing=True`` records events around the exchange (``collective_times()``).

    Step-dependent scalars do not live in kernel arguments: the jitter comes from the ``u``
    buffer (filled per call; default the reference's one ``torch.rand(B, N)`` draw from the CPU
    generator, continued on the device by utils/host_rng.py), Adam's learning rate and bias
    corrections from a 6-float device vector (nerf_amd_adam_step_hyper) fed through a ring of
    pinned buffers.  ``optimizer`` must be ``optim.FusedAdam``.

    ``device_rng=True``: the jitter is drawn inside the kernels by the counter RNG instead (no ``u`` traffic, no host
    work, no wait for the CPU generator's state): seed = ``seed`` + the step count, which travels with the Adam scalars
    (the launches carry NERF_AMD_SEED_IN_MEMORY, so the replayed graph reads the current value); ``ray_id0`` offsets
    the ray ids of this replica, so data-parallel ranks given rank * n_rays draw different jitter.  Same values as the
    eager ``train_step(..., device_rng=True, seed=seed + k, ray_id0=ray_id0)`` at step k (1-based).

    ``step(rays, gt, u=None, decay=1.0)`` returns the loss as a 0-d device tensor (no sync).

    ``rays_from`` = a ``utils.dataload.RayGenerator`` (tables resident in HBM): ``step()`` without rays then runs the
    first lines of the reference's iteration itself (train.py:47-49: ``rg.select(mode, N=batch_size)`` and the
    ``train_imgs[ray_ids]`` gather) on the device.  With ``device_rng=True`` the selection is a node of graph A (counter RNG
    keyed by seed + step, the step counter read from device memory): every replay selects the batch of the NEXT step
    beside its own dX chain -- the selection depends on the counter only, never on the weights -- so it costs the step
    nothing and nothing runs on the host; ``ray_ids`` (the rows the last step trained on) is recomputed on demand.
    Otherwise the ids come from torch's CPU generator continued on the device: the reference's own ``ray_ids`` followed
    by its jitter draw, the generator left exactly where the reference's iteration leaves it.

    ``storage='e4m3'``: what the forward saves for the weight gradients and what the dX chain writes for them travels
    through HBM as 8-bit floats with one power-of-two exponent per 32 features x 32 points instead of bf16 (half the
    bytes of the step's three HBM-bound kernels; the dW products run on the block-scaled 8-bit MFMA).  The forward's
    outputs, the loss and d_raw are bit for bit those of the default; the gradients carry the operands' 8-bit rounding,
    inside the same criterion (a fraction of the reference's own minibatch deviation; tests/test_gpu_storage.py).

    ``background`` (a colour [3] or one per ray [n_rays, 3]) and ``sigma_noise`` (a standard deviation): the head is
    nerf_amd_volume_render_mse_backward_bg, still one launch -- the loss is MSELoss(rgb + (1 - acc) background, gt) and the
    raw density carries Gaussian noise (the reference's open TODO, utils/rendering.py:63).  The background lives in the
    device buffer ``stepper.background``, which the caller may overwrite IN PLACE between replays.  The noise is always the
    counter RNG, with either jitter source: step k (1-based) draws with ``noise_seed`` + k, the step count read from device
    memory -- the eager equivalent is ``train_step(..., noise_seed=noise_seed + k)``.  ``sigma_noise`` is fixed at capture
    and ``stepper.sigma_noise`` is read-only: a schedule on it is a recapture (a new GraphedTrainStep).  Both work with
    ``storage='e4m3'`` and ``buckets=2``: the head sits in front of both.  The dense single step only: the masked,
    hierarchical and guided steppers do not take them.

    ``distortion`` (a weight lambda >= 0, default 0 = off): mip-NeRF 360's distortion loss on the compositor's weights beside
    the MSE (``distortion_loss``).  With lambda > 0 the head is nerf_amd_volume_render_mse_backward_dist,
    still one launch (behind the same background / noise, if any), and the side branch sums its per-ray values
    (nerf_amd_sum_f32): ``stepper.distortion`` is a 0-d device tensor holding the weighted term lambda / (B (tf - tn)) sum_rays D,
    ``step()`` returns the total MSE + term (one fp32 add) -- the eager ``train_step(..., distortion=lambda)`` bit for bit.
    lambda is fixed at capture (``stepper.distortion_weight``, read-only): a schedule on it is a recapture.  The dense single
    step and the guided step only: the masked and hierarchical steppers raise RuntimeError.

    ``controls``: a ``Controls`` -- ``background``, ``sigma_noise``, ``noise_seed`` and ``distortion`` as ONE argument, bit for
    bit the flat keywords (giving both raises ValueError); the masked steppers take the terms through it alone.

    ``check_every`` (default 16, 0 = never): every so many steps the forward's range flag is copied back without
    waiting; a later ``step`` raises FloatingPointError once such a copy shows non-finite values inside the network
    (NaN / inf weights or inputs: a diverged run) -- the reference would show a NaN loss there.

    An optimiser built with ``FusedAdam(..., max_grad_norm=x)`` puts global-norm clipping and the
    non-finite step guard into graph B and the whole-iteration graph: nerf_amd_grad_guard and nerf_amd_adam_step_guarded in
    place of nerf_amd_adam_step_hyper, in every subclass (masked, box, hierarchical, guided, masked guided; the two steppers
    with a per-image table refuse such an optimiser).  The pair sits behind the data-parallel exchange: the norm is that of
    the reduced gradient, the global one, and every rank takes the same decision.  A step whose gradient norm is not finite
    is withheld on the device -- weights, moments and images keep their bits, the next step trains -- with no host
    synchronisation; on the steps ``check_every`` samples the record is copied back without waiting and a later ``step``
    emits one RuntimeWarning naming how many steps were withheld.  ``stepper.grad_norm`` is the optimiser's (a 0-d device
    view of the last norm), ``optimizer.set_max_grad_norm(x)`` takes effect at the next replay without a re-capture.
    """

    _distortion = 0.0            # the distortion term's weight (the dense single step and the guided step only)
    _controls = False            # a background or sigma noise in the head (the dense single step only)
    background, _bg_stride, _sigma_noise, noise_seed = None, 0, 0.0, 0
    _samples = None              # samples per ray of each pass; None: the one pass of N samples
    _capacities = None           # point capacity of each pass (masked passes through ``occupancy``); None: dense passes
    _one_bucket = False          # the two-bucket exchange exists for the dense single step only
    _dense_pass_type = _DensePass        # what a dense pass is: the plain one, or one with more behind its head / dX chain
    _masked_pass_type = _MaskedPass      # what a masked pass is: with its own mark, or behind a launch that marks (_MarkedPass)

    def __init__(self, net, optimizer, n_rays, N, *, tn=2, tf=6, group=None, timing=False, buckets=1,
                 device_rng=False, seed=0, ray_id0=0, check_every=16, rays_from=None, select_mode="train", storage="bf16",
                 background=None, sigma_noise=0.0, noise_seed=0, distortion=0.0, controls=None):
        from . import parallel
        pair = self._samples if self._samples and len(self._samples) == 2 else None
        controls_mod.check_distortion(distortion)        # looked at before the bundle's type, as it always was
        # the flat keywords' meaning here, and the one way the three terms reach a masked pass; the masked and hierarchical
        # steppers inherit this constructor: the flat term cannot slip through them
        c = controls_mod.from_keywords(controls, {"a coarse / fine pair": pair, "an occupancy grid": self._capacities},
                                       background=background, sigma_noise=sigma_noise, noise_seed=noise_seed, distortion=distortion)
        if controls is not None and pair is not None and c.distortion > 0:       # the pair steppers refuse it first (pair)
            controls_mod.refuse_bundle(c, f"the coarse + fine pair ({type(self).__name__}) with the distortion term")
        self._check_modules(net, optimizer)
        self.noise_seed = int(noise_seed) if controls is None else c.noise_seed       # kept whatever is on
        c = controls_mod.resolve(c, int(n_rays), optimizer.flat.device, ray_id0)
        if c is not None:
            self._bg_stride, self._sigma_noise, self._distortion = c.stride, c.std, c.lam
            if c.bg is not None:             # this object's own buffer: the captured head reads it at every replay
                self.background = c.bg.clone()
        self._controls = self.background is not None or self._sigma_noise > 0
        self.net, self.opt, self.group = net, optimizer, group
        if buckets not in (1, 2):
            raise ValueError("buckets must be 1 (one all-reduce between the two graphs, the default) or 2 (overlapped)")
        # group=None is the default process group, as everywhere in parallel.py (train_step(group=None) reduces over it too)
        self.exchange = parallel.collectives_active(group)
        self.bucketed = self.exchange and buckets == 2
        self.timing, self._events = bool(timing), []
        self.device_rng, self.seed, self.ray_id0 = bool(device_rng), int(seed), int(ray_id0)
        self.check_every, self._watch = int(check_every), _StatusWatch()
        self._guard_watch = _GuardWatch() if optimizer.guard is not None else None
        self.B, self.N = int(n_rays), int(N)
        if storage not in ("bf16", "e4m3"):
            raise ValueError("storage must be 'bf16' (the default) or 'e4m3'")
        self.storage, self._e4m3 = storage, storage == "e4m3"
        dev = optimizer.flat.device
        self.dev = dev
        self.rays_from, self.select_mode = rays_from, select_mode
        if rays_from is not None:
            table = rays_from.rays_dataset[select_mode]
            if select_mode not in rays_from.colours:
                raise RuntimeError(f"rays_from has no colour table for mode {select_mode!r}")
            if table.device != dev:
                raise RuntimeError(f"rays_from lives on {table.device}, the module on {dev}")
            if int(table.shape[0]) < self.B:
                raise RuntimeError(f"a batch of {self.B} rays from a table of {int(table.shape[0])}")
        lib = _lib.lib()
        B = self.B
        f32 = dict(dtype=torch.float32, device=dev)
        self.rays = torch.zeros((B, 6), **f32)
        self.rays[:, 5] = -1.0                      # a valid direction: the capture warm-up runs on these buffers
        self.gt = torch.zeros((B, 3), **f32)
        self.u = torch.zeros((B, self.N), **f32)
        self.grads = torch.zeros(optimizer.flat.numel(), **f32)
        self.loss = torch.zeros((), **f32)
        self.hyper = torch.zeros(8, **f32)                 # [lr, b1, b2, eps, 1-b1^t, sqrt(1-b2^t), seed offset (int64)]
        self._alloc_pass_buffers(tn, tf)
        if self._distortion > 0:
            # the head writes coef D per ray; the side branch sums it into `distortion` and adds the MSE (now in its own slot)
            self._t_far, self._dist_coef = float(tf), _distortion_coef(self._distortion, B, tn, tf)
            self._loss_ray, self.distortion = torch.zeros((B,), **f32), torch.zeros((), **f32)
            self.mse = torch.zeros((), **f32)
            self.passes[0].loss = self.mse
        self._ids_next = torch.zeros((B,), dtype=torch.int64, device=dev)      # rays_from: rows of the table (see ray_ids)
        self._ids_cur, self._ids_step, self._primed_for = torch.zeros_like(self._ids_next), -1, -1
        self._select_ws = torch.empty(max(int(lib.nerf_amd_select_workspace_bytes(B)), 256), dtype=torch.uint8, device=dev)
        self._select_ws2 = torch.empty_like(self._select_ws)                    # eager selections beside the captured one
        self.buckets = []                                   # views of the flat gradient vector, in exchange order
        for b in (1, 2):
            first, count = _lib.grad_bucket_range(b)
            self.buckets.append(self.grads[first:first + count])
        self._ring = _HyperRing(dev)
        self._side = torch.cuda.Stream(dev)
        # parameters' .grad are views of the flat gradient vector, as after the eager fused backward
        off = 0
        for p in optimizer.params:
            k = p.numel()
            p.grad = self.grads[off:off + k].view(p.shape)
            off += k
        self._capture()

    def _check_modules(self, net, optimizer):
        from .optim import FusedAdam
        if not isinstance(optimizer, FusedAdam):
            raise RuntimeError("GraphedTrainStep needs optim.FusedAdam (one flat parameter vector)")
        if optimizer.net is not net:
            raise RuntimeError("the optimizer belongs to another module")
        _check_fused_trainable(net.precision)

    @property
    def distortion_weight(self):
        """The weight lambda of the distortion term captured into the head (read-only: a schedule is a new stepper)."""
        return self._distortion

    @property
    def sigma_noise(self):
        """The standard deviation captured into the head (read-only: a schedule is a new GraphedTrainStep)."""
        return self._sigma_noise

    @property
    def _seed_mem(self):
        """The address of this step's seed offset inside the hyper vector (int64 at float slot 6): what a launch with
        NERF_AMD_SEED_IN_MEMORY takes in place of its jitter tensor, and nerf_amd_select_rays as its step counter."""
        return self.hyper.data_ptr() + 24

    def _alloc_pass_buffers(self, tn, tf):
        """``passes`` with their buffers, each pass's module, gradient slice, loss slot and jitter arguments.  A pair
        (coarse, fine) shares ONE jitter draw: ``u`` [B, Nc+Nf] of the reference stream, whose first B*Nc values are
        torch.rand(B,Nc) = ``u_c`` and the rest torch.rand(B,Nf) = ``u_f`` -- the same numbers as the two draws in a row."""
        lib, dev, ptr, B = _lib.lib(), self.dev, _lib.ptr, self.B
        samples = self._samples or (self.N,)
        pair = len(samples) == 2
        self.tbins = _tbins(tn, tf, samples[0], dev)
        if self._capacities is not None:
            occ = self.occupancy
            self._mark_ws = torch.empty(max(int(lib.nerf_amd_occupancy_workspace_bytes(B)), 256), dtype=torch.uint8, device=dev)
            self._counts = torch.zeros(2 * len(samples), dtype=torch.int64, device=dev)       # {live, kept} per pass
            # the grid as the graph sees it: the words' address, the axes as HOST floats, the outside policy
            self._grid = (tuple(occ.resolution), _lib.host_f32x3(occ.lo), _lib.host_f32x3(occ.inv_step),
                          _lib.FLAG_OUTSIDE_EMPTY if occ.outside == "empty" else 0)
            self.passes = [self._masked_pass_type(self, N_, C, self._counts[2 * k:2 * k + 2])
                           for k, (N_, C) in enumerate(zip(samples, self._capacities))]
        else:
            self.passes = [self._dense_pass_type(self, N_, self._e4m3) for N_ in samples]
        # the stratified pass: the buffer, or the counter RNG with this step's seed offset read from device memory
        if self.device_rng:
            jitter = (ptr(self.rays), self._seed_mem, ptr(self.tbins), _lib.FLAG_DEVICE_RNG | _lib.FLAG_SEED_IN_MEMORY,
                      self.seed, self.ray_id0)
        else:
            jitter = (ptr(self.rays), ptr(self.u), ptr(self.tbins), 0, 0, 0)
        self.passes[0].jitter = jitter
        if pair:
            Nc, Nf = samples[0], samples[1] - samples[0]
            self._split_u(Nc, Nf)                   # a pair is a _PairJitter stepper
            self.losses = torch.zeros(2, dtype=torch.float32, device=dev)
            self.ts_f = torch.empty((B, samples[1]), dtype=torch.float32, device=dev)     # the coarse head's output:
            self.passes[1].jitter = (ptr(self.rays), ptr(self.ts_f), None, _lib.FLAG_TS_GIVEN, 0, 0)   # the fine positions
            self._pdf = (None if self.device_rng else ptr(self.u_f), ptr(self.ts_f), Nf)
            self.passes[1].noise_offset = FINE_NOISE_OFFSET     # one noise stream per pass
        off = 0
        for k, (p, net) in enumerate(zip(self.passes, self.opt.nets or (self.net,))):
            n = sum(q.numel() for q in net.parameters())
            p.net, p.grads, p.loss = net, self.grads[off:off + n], self.losses[k] if pair else self.loss
            off += n
        if not pair:         # a single pass's buffers are the stepper's own attributes (bench.py, tools and tests read them)
            for name in ("raw", "ts", "acts", "dys", "posx", "posd", "rgb", "d_raw", "scratch", "scratch8", "pts", "mask",
                         "offsets"):
                if hasattr(self.passes[0], name):
                    setattr(self, name, getattr(self.passes[0], name))

    # ---- the two launch sequences --------------------------------------------------
    def _forward_backward(self, bucket=0):
        """The one forward / backward sequence of every graphed step:

            hyper fetch -> [_before_forward: a subclass's own launches] -> per pass: forward -> head     (main)
            -> fork -> per pass: dX chain  ||  side: per pass encoder rows; per pass loss + dW begin;
                                               [loss sum]; [the next batch's selection]
            -> join -> per pass: dW finish (all products, or with ``bucket`` = 1 only those of the late layers:
                                            _head_gradients adds the rest)

        ONE fork / join inside the captured graph, behind the last head and beside the dX chains."""
        main = torch.cuda.current_stream(self.dev)
        side = self._side
        st, ss = main.cuda_stream, side.cuda_stream
        # first node: this step's scalars (Adam's, the jitter seed offset) from the pinned host ring into `hyper`
        self._ring.fetch(self.hyper, self.dev)
        self._before_forward(st)
        for p in self.passes[:-1]:
            p.forward(st)
            self._coarse_head(p, st)                # writes ts_f, which the next pass's forward (and mark) reads
        self.passes[-1].forward(st)
        self.passes[-1].head(st)
        fork = torch.cuda.Event()
        fork.record(main)                           # behind the last head: what the side branch needs (rgb, d_raw, ts_f, pts) is final
        for p in self.passes:
            p.dx_chain(st)
        side.wait_event(fork)
        # The side branch carries everything the dW products need besides dY -- and nothing else runs beside the forward:
        # a kernel enqueued next to a persistent kernel that fills every CU either delays its start (~10 us per branch at a
        # replayed graph's root) or crawls beside it and slows the compositor behind it.  Order: the encoder rows of a
        # dense pass read this step's rays and jitter, so they come before the selection overwrites the batch.
        for p in self.passes:
            p.encoder_rows(ss)
        for p in self.passes:
            p.loss_and_begin(ss)
        if len(self.passes) == 2:
            with torch.cuda.stream(side):
                torch.add(self.losses[0], self.losses[1], out=self.loss)       # the total, MSE(rgb_c) + MSE(rgb_f)
        if self._distortion > 0:
            _launch("nerf_amd_sum_f32", self._loss_ray, self.distortion, self.B, ss)
            with torch.cuda.stream(side):
                torch.add(self.mse, self.distortion, out=self.loss)            # the total, MSE + the weighted term
        if self.rays_from is not None and self.device_rng:
            # rg.select + the colour gather (train.py:47-49) for the NEXT step, beside the dX chain: this step's rays and
            # colours have been read for the last time (forward or mark + emit, heads on the main branch in front of the
            # fork; encoder rows and losses here), and the selection depends on the step counter only (device memory: every
            # replay selects the batch of step + 1), never on the weights -- so the first lines of the next iteration cost
            # the step nothing.  step() primes the first batch.
            self.rays_from.launch(self.select_mode, self.B, None, self._select_seed(1), self._seed_mem,
                                  self.rays, self.gt, self._ids_next, stream=ss, workspace=self._select_ws)
        main.wait_stream(side)
        for p in self.passes:
            p.finish(bucket, st)

    def _before_forward(self, st):
        """What a stepper enqueues between the hyper fetch and the first forward, on the main branch: nothing here."""

    def _coarse_head(self, c, st):
        """rgb_c, d_raw_c and the fine positions ts_f from the coarse weights, which never reach HBM: one launch.
        ``_pdf`` = (u_f, ts_f, Nf) as pointers; the coarse jitter arguments are ``c.jitter``."""
        c.head(st, self._pdf)

    def _select_seed(self, offset=0):
        """The seed argument of nerf_amd_select_rays for the batch ``offset`` steps after the one the step counter in
        device memory names: the kernel forms (seed ^ KEY) + counter, so the offset goes inside the key.  Replicas
        (distinct ray_id0) draw distinct batches."""
        from .utils.dataload import SELECT_KEY
        m = 0xffffffffffffffff
        base = (self.seed ^ (self.ray_id0 * 0x9E3779B97F4A7C15)) & m
        return ((((base ^ SELECT_KEY) + int(offset)) & m) ^ SELECT_KEY) & m

    def _select_now(self, step, rays, gt, ids):
        """The batch of optimisation step ``step`` (1-based), eagerly: what the graph's prefetch produces one step ahead."""
        self.rays_from.launch(self.select_mode, self.B, None, self._select_seed(step), None, rays, gt, ids, workspace=self._select_ws2)

    @property
    def ray_ids(self):
        """Rows of the table the LAST step trained on (rays_from).  With the selection inside the graph the ids buffer
        already holds the next batch's, so these are recomputed on demand (ids only: three small launches)."""
        if self.rays_from is not None and self.device_rng:
            if self._ids_step != self.opt.step_count:
                self._select_now(self.opt.step_count, None, None, self._ids_cur)
                self._ids_step = self.opt.step_count
            return self._ids_cur
        return self._ids_next

    def _head_gradients(self):
        """The second launch of the bucketed form: the products of layers_0.* (bucket 2)."""
        for p in self.passes:
            p.finish(2, _lib.stream_ptr(self.dev))

    def _update(self):
        """Graph B, and the tail of the whole-iteration graph: the ONE place a graphed stepper launches Adam.  With a guarded
        optimiser (``FusedAdam(max_grad_norm=)``) the norm / verdict launch and the guarded update stand in its place.  Both
        sit behind the data-parallel exchange, so every rank sees the same reduced gradient -- the global norm -- and takes
        the same decision.  The re-pack runs either way (on a withheld step it rewrites the same images)."""
        opt, n, st = self.opt, self.opt.flat.numel(), _lib.stream_ptr(self.dev)
        if opt.guard is None:
            _launch("nerf_amd_adam_step_hyper", opt.flat, self.grads, opt.exp_avg, opt.exp_avg_sq, n, self.hyper, st)
        else:
            _launch("nerf_amd_grad_guard", self.grads, n, opt._guard_ws, opt.guard, st)
            _launch("nerf_amd_adam_step_guarded", opt.flat, self.grads, opt.exp_avg, opt.exp_avg_sq, n, self.hyper, opt.guard, st)
        for net, flat, _ in self._images:                  # every trained module from its slice of the flat vector
            net.repack_from_flat(flat)

    def _set_hyper(self, step):
        from .optim import adam_scalars
        pg = self.opt.param_groups[0]
        self._ring.push(adam_scalars(pg["lr"], pg["betas"], pg["eps"], step), seed_offset=step)

    def _capture(self):
        with torch.cuda.device(self.dev):
            # both images must exist (and be cached) before capture: packing allocates.  Their addresses are baked into
            # the graphs, so this object owns them from here on (_own_images): the module's cache must never replace them
            self._bind_images()
            self._set_hyper(1)
            params0 = self.opt.flat.clone()
            side = torch.cuda.Stream(self.dev)
            side.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(side):                       # warm-up outside capture (lazy inits)
                self._forward_backward()
                if not self._one_bucket:
                    self._head_gradients()
            torch.cuda.current_stream(self.dev).wait_stream(side)
            torch.cuda.synchronize(self.dev)
            # A dead reference cycle that holds device objects (an earlier stepper and its passes refer to each other, with
            # their graphs, streams and pool memory) must not be finalised inside a capture: releasing them calls into the
            # runtime while a stream captures, an error a destructor cannot report -- the process aborts.  torch collects no
            # garbage on entering a capture, so: collect now, and keep the collector off until the last capture has ended.
            import gc
            gc.collect()
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                self.graph_a = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph_a):
                    self._forward_backward(1 if self.bucketed else 0)
                self.graph_a2 = None
                if self.bucketed:
                    self.graph_a2 = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.graph_a2):
                        self._head_gradients()
                self.graph_b = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph_b):
                    self._update()
                # Without an exchange nothing has to happen between the two on most steps: one graph for the whole iteration
                # saves a launch seam (~5-10 us of idle GPU).  Steps that put a status copy / range check between forward and
                # re-pack (check_every) replay the two separate graphs.
                self.graph_ab = None
                if not self.exchange:
                    self.graph_ab = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.graph_ab):
                        self._forward_backward(0)
                        self._update()
            finally:
                if gc_was_on:
                    gc.enable()
            # capture executed nothing, and the warm-up did not touch the parameters
            assert torch.equal(self.opt.flat, params0)
            self._ring.reset()                                   # the warm-up consumed a slot
            # a fresh pair of training images: whatever the warm-up left in their status words is gone
            self._own_images(force=True)

    def _own_images(self, force=False):
        """The two training images the graphs read and re-pack are THIS object's buffers.  If the parameters moved behind
        the graphs' back since the last step (net.load_state_dict to restore a checkpoint, any in-place torch op: their
        versions tell), the module's cache would pack NEW buffers on its next query and free these -- while every replay
        still reads and rewrites them.  So: re-pack from the flat vector (the parameters are views of it) into the
        captured buffers, as new weights (status words cleared), and put exactly these buffers back into the cache."""
        for net, flat, bufs in self._images:
            self._own_images_of(net, flat, bufs, force)

    def _bind_images(self):
        """(module, its slice of the optimizer's flat vector, (forward image, backward image)) per pass."""
        self._images = []
        for p, flat in zip(self.passes, self.opt.slices if self.opt.nets else (self.opt.flat,)):
            p.fwd, p.bwd = p.net.packed_weights(_lib.BF16), p.net.packed_weights(_lib.BF16_BWD)
            self._images.append((p.net, flat, (p.fwd, p.bwd)))
        self._packed_fwd, self._packed_bwd = self._images[0][2]

    def _own_images_of(self, net, flat, bufs, force):
        from .utils.nets import _Packed
        dev = self.dev
        params = net._param_list()
        stamp = tuple((p.data_ptr(), p._version) for p in params)
        ents = [net._packed.get((dev, c)) for c in (_lib.BF16, _lib.BF16_BWD)]
        if not force and all(e is not None and e.stamp == stamp and e.buf is b for e, b in zip(ents, bufs)):
            return
        off = 0
        for p in params:                                   # FusedAdam made them views of its flat vector; still true?
            if p.data_ptr() != flat.data_ptr() + 4 * off:
                raise RuntimeError("a parameter no longer lives in the optimizer's flat vector (its .data was replaced): "
                                   f"build a new FusedAdam and {type(self).__name__}")
            off += p.numel()
        for code, buf in zip((_lib.BF16, _lib.BF16_BWD), bufs):
            _lib.launch("nerf_amd_pack_weights", flat, buf, code, dev=dev)
            net._packed[(dev, code)] = _Packed(stamp, buf)
        net.drop_packed(dev, keep=(_lib.BF16, _lib.BF16_BWD))

    # ---- one iteration -------------------------------------------------------------
    def step(self, rays=None, gt=None, u=None, decay=1.0):
        from . import parallel
        if (rays is None) != (gt is None):
            raise RuntimeError("step(): rays and gt come together (or neither, with rays_from)")
        if rays is None and self.rays_from is None:
            raise RuntimeError("step() without rays needs GraphedTrainStep(..., rays_from=<utils.dataload.RayGenerator>)")
        if rays is not None and (rays.shape != self.rays.shape or gt.shape != self.gt.shape):
            raise RuntimeError(f"GraphedTrainStep was captured for rays {tuple(self.rays.shape)}, gt {tuple(self.gt.shape)}")
        self._watch.raise_if_diverged("step")
        self._note_withheld()
        self._own_images()
        if rays is None and self.device_rng and self._primed_for != self.opt.step_count + 1:
            # the first step (or one after the step counter was moved by hand): the graph prefetches batch k + 1 while
            # step k runs, so batch k has to be there before the first replay
            self._select_now(self.opt.step_count + 1, self.rays, self.gt, self._ids_next)
        if rays is not None:
            if self.rays_from is not None and self.device_rng:
                raise RuntimeError("this GraphedTrainStep selects its rays inside the captured graph (rays_from, device_rng=True): "
                                   "step() takes no rays")
            self.rays.copy_(rays, non_blocking=True)
            self.gt.copy_(gt, non_blocking=True)
        session = None
        try:
            if self.device_rng:
                if u is not None:
                    raise RuntimeError("this GraphedTrainStep draws its jitter on the device (device_rng=True): u must be None")
            else:
                from .utils import host_rng
                if rays is None and host_rng.host_fallback():
                    self.rays_from.select_batch(self.select_mode, self.B, out=(self.rays, self.gt, self._ids_next))
                elif rays is None:
                    # the reference's iteration on torch's CPU stream, continued on the device: randperm(n)[:B] (the n - 1 - B
                    # draws nobody looks at are jumped over), the two gathers, then -- same stream -- the jitter draw
                    session = host_rng.GeneratorSession(self.dev)
                    drawn = self.rays_from.select_from_session(session, self.select_mode, self.B, self.rays, self.gt, self._ids_next,
                                                               workspace=self._select_ws,
                                                               jitter=(self.B, self.N, self.u) if u is None else None)
                    if drawn is not None:
                        u = self.u                       # the jitter came with the selection (one jump launch for both)
                if u is self.u:
                    pass
                elif u is None:
                    # the reference's one draw per call from torch's CPU generator, continued on the device; the generator is
                    # made current again (session.finish: a wait for the generator kernels alone) once the whole step is
                    # enqueued behind it, so the host never waits for the previous step here
                    if host_rng.host_fallback():
                        self.u.copy_(torch.rand(self.B, self.N), non_blocking=False)
                    else:
                        session = session or host_rng.GeneratorSession(self.dev)
                        session.rand(self.B, self.N, out=self.u)
                else:
                    self.u.copy_(u, non_blocking=True)
            return self._enqueue_step(decay)
        finally:
            if session is not None:
                session.finish()

    def _enqueue_step(self, decay):
        """``opt.step_count`` counts the steps ATTEMPTED: it advances here, in front of the replay, and the scalars pushed are
        that count's.  If ``replay()`` itself raises, or anything behind it does before the ring's ``launched``, the count
        stays advanced -- time passes on such a step as it does on a step the gradient guard withholds -- and the next
        ``_set_hyper`` finds the ring's step still open and takes the slot index from the device counter (_HyperRing), so
        the next replay runs with its own scalars whether the failed one was enqueued or not."""
        from . import parallel
        self.opt.step_count += 1
        self._set_hyper(self.opt.step_count)
        watch = bool(self.check_every) and self.opt.step_count % self.check_every == 0
        whole = self.graph_ab is not None and not watch
        (self.graph_ab if whole else self.graph_a).replay()
        self._ring.launched(self.dev)
        if self.rays_from is not None and self.device_rng:
            self._primed_for = self.opt.step_count + 1          # graph A left the next step's batch in the buffers
        if watch:
            # behind the forward, in front of graph B's re-pack (which clears the flag for the next step)
            for _, _, bufs in self._images:
                self._watch.push(bufs[0], self.opt.step_count)
            # the reference's |x| > 1 warning (utils/xyz.py:8-9) on the batch in the buffers (with the selection inside the
            # graph that is already the next step's), verdict raised lazily
            self._range_check()
        if self.bucketed:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if self.timing else None
            if ev:
                ev[0].record()                                           # late gradients done, exchange starts
            h1 = parallel.allreduce_start_(self.buckets[0], group=self.group)
            self.graph_a2.replay()                                       # head gradients, beside the first exchange
            if ev:
                ev[1].record()
            h2 = parallel.allreduce_start_(self.buckets[1], group=self.group)
            parallel.allreduce_wait_(h1)
            parallel.allreduce_wait_(h2)
            if ev:
                ev[2].record()
                self._events.append(ev)
        elif self.exchange:
            # buckets=1: the whole 2.38 MB vector in one all-reduce between the two graphs, fully exposed
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if self.timing else None
            if ev:
                ev[0].record()
            parallel.allreduce_flat_(self.grads, group=self.group)
            if ev:
                ev[1].record()
                self._events.append([ev[0], ev[0], ev[1]])
        if not whole:
            self.graph_b.replay()
        if watch and self.opt.guard is not None:
            self._guard_watch.push(self.opt.guard, self.opt.step_count)      # behind graph B, which filled it
        # graph B re-packed the two training images; any other image of the module (fp16 / fp32 inference) is now
        # stale -- and the kernels wrote through the flat buffer, so the parameters' versions did not move
        for net, _, _ in self._images:
            net.drop_packed(self.dev, keep=(_lib.BF16, _lib.BF16_BWD))
        if decay != 1.0:
            for pg in self.opt.param_groups:
                pg["lr"] = pg["lr"] * decay
        return self.loss

    __call__ = step

    @property
    def grad_norm(self):
        """The optimiser's ``grad_norm``: the last step's gradient norm before clipping, a 0-d device view (no sync); None
        for an optimiser without ``max_grad_norm``."""
        return self.opt.grad_norm

    def _note_withheld(self):
        """First thing in ``step``: one RuntimeWarning per completed sample of the guard record (taken on the steps
        ``check_every`` samples) whose skipped counter has risen."""
        import warnings
        for step, k in (self._guard_watch.risen() if self._guard_watch is not None else ()):
            warnings.warn(f"{type(self).__name__}: the gradient guard withheld {k} training step{'s' if k != 1 else ''} up to step "
                          f"{step} (a gradient norm that was not finite: NaN / inf in the batch or the gradients); weights and "
                          "moments kept their values on those steps", RuntimeWarning, stacklevel=3)

    def _range_check(self):
        """The reference's |x| > 1 warning on the stratified pass's first / last samples (the finer passes lie between)."""
        from .utils.xyz import range_check_rays
        first = self.passes[0]
        _, jit, _, flags, seed, rid = first.jitter
        range_check_rays(self.rays, jit, self.tbins, flags, seed, rid, first.N)

    def reset_timing(self):
        """Forget the exchange events recorded so far (warm-up steps: the first collective creates the communicator)."""
        self._events = []

    def collective_times(self):
        """(span_ms, exposed_ms) averaged over the steps recorded with timing=True: from the end of the late-layer
        gradients to both buckets reduced, and the part of it behind the end of the head-gradient launch (what the
        step actually waits for).  Synchronises; clears the record."""
        if not self._events:
            return None
        torch.cuda.synchronize(self.dev)
        span = sum(e[0].elapsed_time(e[2]) for e in self._events) / len(self._events)
        exposed = sum(e[1].elapsed_time(e[2]) for e in self._events) / len(self._events)
        self._events = []
        return span, exposed


class _TableAdam:
    """The optimiser of a per-image table (``table`` [M,6]) trained beside the network inside the captured graph: an Adam of
    its own -- nerf_amd_adam_step_hyper on (table, ``grad``) -- with scalars of its own (``optim.adam_scalars``: the update
    is Adam's for exactly the fp32 betas the kernel holds), fed through a ring of its own.  ``steps`` counts the steps
    attempted, as ``FusedAdam.step_count`` does: ``push`` advances it in front of the replay and writes that step's scalars."""

    def __init__(self, table, lr, betas, eps):
        self.table, self.lr, self.eps, self.steps = table, float(lr), float(eps), 0
        self.betas = tuple(float(torch.tensor(float(b), dtype=torch.float32)) for b in betas)
        self.grad = torch.zeros_like(table, requires_grad=False)
        self.m, self.v = torch.zeros_like(self.grad), torch.zeros_like(self.grad)
        self.hyper, self.ring = torch.zeros(8, dtype=torch.float32, device=table.device), _HyperRing(table.device)

    def push(self):
        from .optim import adam_scalars
        self.steps += 1
        self.ring.push(adam_scalars(self.lr, self.betas, self.eps, self.steps))

    def update(self):
        _launch("nerf_amd_adam_step_hyper", self.table, self.grad, self.m, self.v, self.table.numel(), self.hyper,
                _lib.stream_ptr(self.table.device))


def _table_adam_attr(name):
    """A stepper's public name for a field of its table's optimiser (``camera_lr`` = ``_adam2.lr``, assignable)."""
    return property(lambda self: getattr(self._adam2, name), lambda self, value: setattr(self._adam2, name, value))


class _TableTrainStep(GraphedTrainStep):
    """What the steppers with a per-image table share.  The table (``_table``: its attribute of the object the stepper is
    given) is trained by ``_adam2`` (a _TableAdam) inside the captured graph, its images are the images of ``rays_from``'s
    table, and the stepper's first launch keeps the ids a step ran on in ``_ids_used``.  ``_words``: what differs between
    the steppers' messages (``spans`` is formatted with the object); ``_baked_now()``: the addresses the graph holds."""

    def _bind_table(self, obj, kind, optimizer, n_rays, rays_from, select_mode, group, lr, betas, eps):
        """The refusals the table steppers share, in their order, before any launch or RNG draw; then the table's optimiser."""
        from . import parallel
        name, w = type(self).__name__, self._words
        if parallel.collectives_active(group):
            raise RuntimeError(f"{name} trains on one replica: the {w['gradient']} gradient has no exchange yet")
        if not isinstance(obj, kind):
            raise RuntimeError(w["type"])
        if rays_from is None:
            raise RuntimeError(f"{name} {w['why']} the ids of a selection: rays_from=<RayGenerator> is required")
        if select_mode not in rays_from.colours:
            raise RuntimeError(f"rays_from has no colour table for mode {select_mode!r}")
        rows, table = int(rays_from.rays_dataset[select_mode].shape[0]), getattr(obj, self._table)
        if rows != obj.n_rays:
            raise RuntimeError(f"the table of rays_from holds {rows} rays, {w['spans'].format(obj)} = {obj.n_rays}")
        if table.device != optimizer.flat.device:
            raise RuntimeError(f"{w['lives']} on {table.device}, the module on {optimizer.flat.device}")
        if getattr(optimizer, "guard", None) is not None:
            # the table's own Adam is not guarded: a network step withheld beside a table step taken would be worse than either
            raise RuntimeError(f"{name} does not take an optimizer with max_grad_norm: the {w['gradient']} table's own Adam is not "
                               "guarded yet (build FusedAdam without max_grad_norm)")
        self._adam2 = _TableAdam(table, lr, betas, eps)
        self._ids_used = torch.zeros((int(n_rays),), dtype=torch.int64, device=table.device)

    @property
    def ray_ids(self):
        """Rows of the table the LAST step trained on: the copy the stepper's first launch kept."""
        return self._ids_used

    def _before_forward(self, st):
        """The table's scalars behind the step's own; the subclass's first launch follows."""
        self._adam2.ring.fetch(self._adam2.hyper, self.dev)

    def _set_hyper(self, step):
        super()._set_hyper(step)
        self._adam2.push()

    def _update(self):
        super()._update()
        self._adam2.update()

    def _capture(self):
        steps = self._adam2.steps
        super()._capture()
        self._adam2.ring.reset()                     # the warm-up consumed a slot ...
        self._adam2.steps = steps                    # ... and was no step

    def _enqueue_step(self, decay):
        loss = super()._enqueue_step(decay)
        self._adam2.ring.launched(self.dev)
        return loss

    def _table_step(self, rays, gt, u, decay, table_decay):
        name, w = type(self).__name__, self._words
        if rays is not None or gt is not None:
            raise RuntimeError(f"{name} {w['why']} the selected ids: step() takes no rays")
        if self._baked_now() != self._baked:
            raise RuntimeError(f"{w['baked']} replaced: baked into the captured graph (write in place, or build a new {name})")
        loss = super().step(None, None, u=u, decay=decay)
        self._adam2.lr *= float(table_decay)
        return loss


class _IdsOnlySelection:
    """``rays_from`` as GraphedCameraTrainStep hands it to its base: every selection still writes the colours and the ids, and
    no rays (nerf_amd_select_rays with rays_out = NULL) -- the stepper forms them itself, from the ids and its cameras."""

    def __init__(self, rg):
        self._rg = rg

    def __getattr__(self, name):
        return getattr(self._rg, name)

    def launch(self, mode, B, draws, seed, seed_mem, rays, gt, ids, stream=None, workspace=None):
        self._rg.launch(mode, B, draws, seed, seed_mem, None, gt, ids, stream=stream, workspace=workspace)


class _CameraPass(_DensePass):
    """The dense pass with the pose gradient behind its dX chain, on the main branch: d loss / d rays from the same dY
    (nerf_amd_input_gradients on the flat fp32 parameters, the step's rays and positions), then its reduction to one
    6-vector per image (nerf_amd_camera_rays_backward on the ids the rays were formed from)."""

    def dx_chain(self, st):
        super().dx_chain(st)
        s = self.step
        _launch("nerf_amd_input_gradients", self.dys, s.opt.flat, None, s.rays, self.ts, s._dv, s.d_rays, self.P, self.N, st)
        s.cameras._launch_backward(s.cameras.xi, s._ids_used, s.d_rays, s.camera_grad, stream=st)


class GraphedCameraTrainStep(_TableTrainStep):
    """GraphedTrainStep with a camera optimiser inside the captured graph: the rays of every step are
    formed on the device from ``cameras`` (``utils.cameras.CameraRefinement``: stored poses and the learnable corrections
    ``cameras.xi`` [M,6]) and the ids the selection left, and ``xi`` is trained beside the network by an Adam of its own.

        graph A: hyper fetch -> camera hyper fetch -> camera rays (nerf_amd_camera_rays: writes ``rays`` and keeps a copy of
                 the ids) -> forward -> head -> dX chain -> input gradients (nerf_amd_input_gradients: ``d_rays``) -> camera
                 backward (nerf_amd_camera_rays_backward: ``camera_grad`` = d loss / d xi) -> dW products; the side branch
                 is GraphedTrainStep's, its selection of the next batch writing colours and ids only
        graph B: Adam -> re-pack -> Adam on (xi, camera_grad) with the camera's own scalars (nerf_amd_adam_step_hyper)

    The rays of step k see the ``xi`` step k - 1 wrote -- which is why they cannot come from the one-step-ahead selection.
    ``rays_from`` is required (a ``RayGenerator`` with colours whose table has the cameras' M H W rows); ``step()`` takes no
    rays.  ``camera_lr``, ``camera_betas`` (held rounded to fp32, the kernel's format), ``camera_eps``: the camera Adam's;
    ``step(camera_decay=)`` multiplies ``camera_lr`` as ``decay`` does the network's rate.  ``camera_grad`` [M,6] is the last
    step's gradient, ``cameras.xi`` is live, ``ray_ids`` are the rows the last step trained on.  Both jitter sources work.
    d loss / d rays is what nerf_amd_input_gradients gives, as on the eager fused path (the compositor's |d_hat| factor is 1
    and carries none).  The addresses of ``cameras.xi`` and of the stored poses are baked into the graph: write them in place
    (``load_state_dict`` does); ``step`` raises if either tensor was replaced.

    Refused (RuntimeError, before any launch or RNG draw): ``storage='e4m3'`` (nerf_amd_input_gradients reads bf16 dY),
    ``buckets=2``, a process group that exchanges gradients (``camera_grad`` would need an exchange of its own),
    ``background`` / ``sigma_noise`` / ``distortion``, an optimizer built with ``max_grad_norm`` (the camera Adam is not guarded)."""

    _one_bucket = True
    _dense_pass_type = _CameraPass               # the dense pass and its buffers, the pose gradient behind its dX chain
    _table = "xi"
    _words = dict(gradient="camera", type="cameras must be a utils.cameras.CameraRefinement", why="forms its rays from",
                  spans="the cameras span {0.M} x {0.H} x {0.W}", lives="the cameras live",
                  baked="cameras.xi or the stored poses were")
    camera_lr, camera_betas, camera_eps, camera_steps, camera_grad = map(_table_adam_attr, ("lr", "betas", "eps", "steps", "grad"))

    def __init__(self, net, optimizer, n_rays, N, cameras, *, rays_from=None, camera_lr=1e-3, camera_betas=(0.9, 0.999),
                 camera_eps=1e-8, select_mode="train", group=None, buckets=1, storage="bf16", background=None, sigma_noise=0.0,
                 distortion=0.0, **kw):
        from .utils.cameras import CameraRefinement
        from .utils.box import refuse_box
        refuse_box(kw.pop("box", None), "GraphedCameraTrainStep")
        controls_mod.refuse_bundle(kw.pop("controls", None), "GraphedCameraTrainStep")
        if storage != "bf16":
            raise RuntimeError("GraphedCameraTrainStep: storage='e4m3' is not served (nerf_amd_input_gradients reads bf16 dY)")
        if buckets != 1:
            raise RuntimeError("GraphedCameraTrainStep: one exchange bucket only (buckets=1)")
        controls_mod.refuse_flat(type(self).__name__, background, sigma_noise, distortion)
        self._bind_table(cameras, CameraRefinement, optimizer, n_rays, rays_from, select_mode, group, camera_lr, camera_betas,
                         camera_eps)
        self.cameras = cameras
        self._baked = self._baked_now()
        f32 = dict(dtype=torch.float32, device=cameras.xi.device)
        self.d_rays = torch.zeros((int(n_rays), 6), **f32)
        self._dv = torch.empty((int(n_rays) * int(N), 6), **f32)
        super().__init__(net, optimizer, n_rays, N, rays_from=_IdsOnlySelection(rays_from), select_mode=select_mode, group=group, **kw)

    def _baked_now(self):
        return self.cameras.xi.data_ptr(), self.cameras.poses0.data_ptr()

    def _before_forward(self, st):
        super()._before_forward(st)
        self.cameras._launch_rays(self.cameras.xi, self._ids_next, self._ids_used, self.rays, stream=st)

    def step(self, rays=None, gt=None, u=None, decay=1.0, camera_decay=1.0):
        return self._table_step(rays, gt, u, decay, camera_decay)

    __call__ = step


class _AppearancePass(_DensePass):
    """The dense pass with the loss behind the per-image colour correction: the affine head (compositor + the map + MSE
    gradient + the map's backward + compositor backward, ONE kernel: nerf_amd_volume_render_mse_backward_affine; ``rgb`` is
    c', so the side branch's loss is the MSE behind the correction), and the reduction of the rays' rows of d loss / d theta
    to one per image (nerf_amd_appearance_reduce on the ids the rows were gathered by) on the main branch."""

    def _reduce(self, st):
        s = self.step
        a = s.appearance
        _launch("nerf_amd_appearance_reduce", s._g_theta_ray, s._ids_used, a.HW, a.theta, a.reg, a._frozen_arg,
                s.appearance_grad, s.B, a.M, st)

    def head(self, st, pdf=None):
        s, (rays, *_) = self.step, self.jitter
        _launch("nerf_amd_volume_render_mse_backward_affine", self.raw, self.ts, rays, s.gt, s._theta_ray, 6,
                self.rgb, s._g_theta_ray, self.d_raw, s.B, self.N, st)
        if s._reduce_behind == "head":
            self._reduce(st)

    def dx_chain(self, st):
        super().dx_chain(st)
        if self.step._reduce_behind == "dx":
            self._reduce(st)


class GraphedAppearanceTrainStep(_TableTrainStep):
    """GraphedTrainStep with a per-image colour correction inside the captured graph: the loss of every
    step is ``MSELoss((1 + a) rgb + b, gt)`` with the row (a, b) of each ray's image (``appearance``: a
    ``utils.appearance.AppearanceCorrection``, ``appearance.theta`` [M,6]), and ``theta`` is trained beside the network by an
    Adam of its own.

        graph A: hyper fetch -> appearance hyper fetch -> gather (nerf_amd_appearance_gather: one row of theta per ray, and a
                 copy of the ids) -> forward -> affine head (nerf_amd_volume_render_mse_backward_affine) -> dX chain -> reduce
                 (nerf_amd_appearance_reduce: ``appearance_grad`` = d loss / d theta, with the ridge and the frozen rows) -> dW
                 products; the side branch is GraphedTrainStep's, its selection of the next batch writing the shared id buffer
                 while this step reduces by its own copy
        graph B: Adam -> re-pack -> Adam on (theta, appearance_grad) with scalars of its own (nerf_amd_adam_step_hyper)

    ``rays_from`` is required (a ``RayGenerator`` with colours whose table has the correction's M HW rows): the image of a ray
    is its row // HW, so ``step()`` takes no rays.  ``appearance_lr``, ``appearance_betas`` (held rounded to fp32, the kernel's
    format), ``appearance_eps``: the second Adam's; ``step(appearance_decay=)`` multiplies ``appearance_lr`` as ``decay`` does
    the network's rate.  ``step`` returns the MSE behind the correction.  ``appearance_grad`` [M,6] is the last step's gradient,
    ``appearance.theta`` is live, ``ray_ids`` are the rows the last step trained on.  Both jitter sources work, and so does
    ``storage='e4m3'`` (the head does not touch the storage form).  The address of ``appearance.theta`` is baked into the graph:
    write it in place (``load_state_dict`` does); ``step`` raises if the tensor was replaced.

    Refused (RuntimeError, before any launch or RNG draw): a process group that exchanges gradients (``appearance_grad`` has no
    exchange yet), ``background`` / ``sigma_noise`` / ``distortion``, an ``appearance`` whose M HW is not the table's length or
    that lives on another device, an optimizer built with ``max_grad_norm`` (the second Adam is not guarded).  The masked,
    hierarchical, guided and camera steppers do not take a correction."""

    _reduce_behind = "dx"        # where the reduction sits on the main branch: behind the "dx" chain or behind the "head"
    _dense_pass_type = _AppearancePass           # the dense pass and its buffers, the loss behind the correction
    _table = "theta"
    _words = dict(gradient="appearance", type="appearance must be a utils.appearance.AppearanceCorrection",
                  why="finds a ray's image from", spans="the correction spans {0.M} x {0.HW}", lives="the correction lives",
                  baked="appearance.theta was")
    appearance_lr, appearance_betas, appearance_eps, appearance_steps, appearance_grad = map(
        _table_adam_attr, ("lr", "betas", "eps", "steps", "grad"))

    def __init__(self, net, optimizer, n_rays, N, appearance, *, rays_from, appearance_lr=1e-3, appearance_betas=(0.9, 0.999),
                 appearance_eps=1e-8, select_mode="train", group=None, **kw):
        from .utils.appearance import AppearanceCorrection
        from .utils.box import refuse_box
        refuse_box(kw.pop("box", None), "GraphedAppearanceTrainStep")
        controls_mod.refuse_bundle(kw.pop("controls", None), "GraphedAppearanceTrainStep")
        controls_mod.refuse_flat(type(self).__name__, kw.get("background"), kw.get("sigma_noise"), kw.get("distortion"))
        self._bind_table(appearance, AppearanceCorrection, optimizer, n_rays, rays_from, select_mode, group, appearance_lr,
                         appearance_betas, appearance_eps)
        self.appearance = appearance
        self._baked = self._baked_now()
        f32 = dict(dtype=torch.float32, device=appearance.theta.device)
        self._theta_ray, self._g_theta_ray = torch.zeros((int(n_rays), 6), **f32), torch.zeros((int(n_rays), 6), **f32)
        super().__init__(net, optimizer, n_rays, N, rays_from=rays_from, select_mode=select_mode, group=group, **kw)

    def _baked_now(self):
        return self.appearance.theta.data_ptr()

    def _before_forward(self, st):
        a = self.appearance
        super()._before_forward(st)
        _launch("nerf_amd_appearance_gather", a.theta, self._ids_next, self._ids_used, a.HW, self._theta_ray, self.B, a.M, st)

    def step(self, rays=None, gt=None, u=None, decay=1.0, appearance_decay=1.0):
        return self._table_step(rays, gt, u, decay, appearance_decay)

    __call__ = step


class _MaskedSteps:
    """What the two masked steppers share (listed in front of their stepper base): the refusals, the grid and the capacities,
    and the overflow report -- ``counts`` on the device is int64 {live, kept} per pass, copied back every ``check_every``
    steps without waiting."""

    _one_bucket = True

    def _refuse(self, storage, buckets):
        name = type(self).__name__
        if storage != "bf16":
            raise ValueError(f"{name} keeps its operands in bf16: storage={storage!r} is not supported")
        if buckets != 1:
            raise ValueError(f"{name} exchanges its gradients in one bucket: buckets must be 1")

    def _bind_grid(self, nets, samples, B, optimizer, occupancy, capacity):
        """Checks the modules, the grid and the capacity argument (one value, or a pair (C_c, C_f) for two passes) in this
        order and, if nothing raised, keeps them."""
        from .utils import occupancy as occ_mod
        for net, N_ in zip(nets, samples):
            occ_mod.check_trainable(occupancy, net, torch.empty(0), N_)
        self._check_modules(nets[0] if len(nets) == 1 else nets, optimizer)
        if len(nets) == 1:
            self._capacities = (_capacity_points(capacity, B * samples[0], "capacity"),)
        else:
            if isinstance(capacity, (str, bytes)) or not hasattr(capacity, "__len__") or len(capacity) != 2:
                raise TypeError("capacity must be a pair (C_c, C_f), each an int (points) or a float (fraction of the pass's samples)")
            self._capacities = tuple(_capacity_points(c, B * N_, f"the {w} capacity")
                                     for c, N_, w in zip(capacity, samples, ("coarse", "fine")))
        if occupancy.words.device != optimizer.flat.device:
            raise RuntimeError(f"the occupancy grid lives on {occupancy.words.device}, the module on {optimizer.flat.device}")
        self.occupancy = occupancy
        self._words_ptr = occupancy.words.data_ptr()
        self._counts_watch = _CountsWatch(width=2 * len(nets))
        self.last_stats, self.overflow_steps = None, 0

    def _range_check(self):
        """Runs behind graph A on every ``check_every``-th step: the reference's |x| > 1 warning on the points the networks
        were asked about (the pad point is in range), and the copy of ``counts`` the overflow report reads."""
        from .utils.xyz import range_check_values
        for p in self.passes:
            range_check_values(p.pts)
        self._counts_watch.push(self._counts, self.opt.step_count)

    def _stats(self, step, values):
        per = [{"samples": self.B * p.N, "live": values[2 * k], "kept": values[2 * k + 1], "capacity": p.P}
               for k, p in enumerate(self.passes)]
        return {"step": step, **per[0]} if len(per) == 1 else {"step": step, "coarse": per[0], "fine": per[1]}

    def _note(self, done, stacklevel):
        import warnings
        for step, *values in done:
            self.last_stats = s = self._stats(step, values)
            per = {None: s} if "live" in s else {name: s[name] for name in ("coarse", "fine")}
            over = {name: q for name, q in per.items() if q["live"] > q["capacity"]}
            if not over:
                continue
            self.overflow_steps += 1
            if None in over:
                what = (f"step {step} had {s['live']} live samples for a capacity of {s['capacity']} points; the last "
                        f"{s['live'] - s['kept']} (ray-major order) were treated as dead")
            else:
                what = f"step {step}: " + "; ".join(
                    f"the {name} pass had {q['live']} live samples for a capacity of {q['capacity']} points, the last "
                    f"{q['live'] - q['kept']} (ray-major order) were treated as dead" for name, q in over.items())
            warnings.warn(f"{type(self).__name__}: {what}.  Build a stepper with a larger capacity.", RuntimeWarning,
                          stacklevel=stacklevel)

    def counts(self):
        """The report of the latest step in the shape of ``last_stats``, read now (synchronises); pending reports are
        delivered first."""
        self._note(self._counts_watch.poll(wait=True), 3)
        return self._stats(self.opt.step_count, [int(v) for v in self._counts.cpu()])

    def _watch_grid(self):
        """First thing in ``step``: the grid is still the captured one; completed overflow reports are delivered."""
        if self.occupancy.words.data_ptr() != self._words_ptr:
            raise RuntimeError("the occupancy grid's words tensor was replaced: its address is baked into the captured graph "
                               f"(TrainingOccupancyGrid.update writes in place); build a new {type(self).__name__}")
        self._note(self._counts_watch.poll(), 4)


class GraphedMaskedTrainStep(_MaskedSteps, GraphedTrainStep):
    """``train_step(..., occupancy=)`` as captured hipGraphs: GraphedTrainStep with its one pass
    masked -- DESIGN.md section 14.  The live count P' of a batch
    never reaches the host on the step's path: the graph is captured for a fixed point ``capacity`` C (an int number of
    points, or a float fraction of n_rays * N; NO default -- what is safe depends on the scene and the grid), every network
    kernel runs on exactly C points, and the rows no live sample owns are inert (include/nerf_amd.h: pad points in,
    zero d_raw out, so they add exact zeros to every gradient).

        graph A: hyper fetch -> mark + scan (nerf_amd_occupancy_mark) -> capped emit (nerf_amd_occupancy_points_capped:
                 pts[C, 6], counts) -> training forward on the C points -> masked head (compositor + MSE gradient +
                 compositor backward, ONE kernel: nerf_amd_volume_render_masked_mse_backward) -> dX chain -> dW products;
                 the side branch beside the dX chain is GraphedTrainStep's
        graph B and the all-reduce seam: GraphedTrainStep's, unchanged (one exchange bucket).

    With P' <= C the step is the eager masked step.  With P' > C (an overflow) the live samples of global rank >= C -- the
    tail in ray-major order -- are treated as dead: a well-defined step under a stricter mask, reported, never silent:
    every ``check_every`` steps ``counts`` is copied back without waiting; ``last_stats`` = {'step', 'samples', 'live',
    'kept', 'capacity'} of the latest completed copy, an observed overflow raises a RuntimeWarning (``overflow_steps``
    counts them), ``counts()`` reads the latest step's now (one sync).  To change the capacity build a new stepper on the
    same optimizer (it holds the state).

    ``occupancy``: an ``OccupancyGrid`` / ``TrainingOccupancyGrid`` on the module's device.  The address of its ``words``
    is baked into the graph (``step`` raises if the tensor was replaced); ``TrainingOccupancyGrid.update`` writes the bits
    in place, so an update between two replays simply takes effect.  Jitter and ``step`` as GraphedTrainStep.  bf16 storage,
    N <= 512, the default network.

    ``controls``: a ``Controls`` -- with any term on the head is
    nerf_amd_volume_render_masked_mse_backward_dist, still one launch under the same clamp: the loss behind
    ``stepper.background`` (the stepper's own buffer, overwritable in place between replays), Gaussian noise on the live rows
    keyed by ``noise_seed`` + the step count read from device memory (step k draws what the eager masked step draws with
    ``noise_seed + k``), and the distortion term, whose per-ray values the side branch sums into ``stepper.distortion`` while
    ``step()`` returns the total -- GraphedTrainStep's machinery.  Without it the step is the one it was, kernel for kernel.
    The flat ``distortion=`` keyword keeps refusing here."""

    def __init__(self, net, optimizer, n_rays, N, occupancy, capacity, *, tn=2, tf=6, group=None, device_rng=False, seed=0,
                 ray_id0=0, check_every=16, rays_from=None, select_mode="train", buckets=1, storage="bf16", distortion=0.0,
                 controls=None):
        controls_mod.check_distortion(distortion, {"an occupancy grid": occupancy})
        controls = controls_mod.bundle(controls)
        self._refuse(storage, buckets)
        B, N_ = int(n_rays), int(N)
        if B < 1 or N_ < 1:
            raise ValueError(f"GraphedMaskedTrainStep needs n_rays >= 1 and N >= 1 (got {n_rays}, {N})")
        self._bind_grid((net,), (N_,), B, optimizer, occupancy, capacity)
        self.capacity = self._capacities[0]
        super().__init__(net, optimizer, B, N_, tn=tn, tf=tf, group=group, device_rng=device_rng, seed=seed, ray_id0=ray_id0,
                         check_every=check_every, rays_from=rays_from, select_mode=select_mode, controls=controls)

    def step(self, rays=None, gt=None, u=None, decay=1.0):
        self._watch_grid()
        return super().step(rays, gt, u=u, decay=decay)

    __call__ = step


class _BoxSteps:
    """What the two scene-box steppers share (listed in front of their stepper base): the stepper's own
    jitter arguments become the PLACEMENT's (on the unit bins ``tbins01``; with ``device_rng`` the seed offset is read from
    device memory, as before), the one pass reads the placed positions ``ts_box`` under NERF_AMD_TS_GIVEN, and
    nerf_amd_box_positions is one more node of graph A in front of the forward.  ``box.lo`` / ``box.hi`` are baked into the
    graph by value: a SceneBox is frozen, another box is another stepper.
    With a ``GridSpan`` the node is nerf_amd_span_positions and what is baked in is the ADDRESS of the
    span's grid's ``words``: ``TrainingOccupancyGrid.update`` writes the bits in place, so an update between two replays
    simply takes effect, and ``step`` raises if that tensor was replaced."""

    def _bind_box(self, box, N, tn, tf):
        from .utils.box import GridSpan, check_box, check_interval
        if check_box(box) is None:
            raise TypeError(f"{type(self).__name__} needs a utils.box.SceneBox or GridSpan")
        check_interval(N, tn, tf)
        self.box, self._box_interval = box, (float(tn), float(tf))
        self._span_words_ptr = box.occupancy.words.data_ptr() if isinstance(box, GridSpan) else None

    def _watch_span(self):
        """First thing in ``step``: the span's grid is still the captured one."""
        if self._span_words_ptr is not None and self.box.occupancy.words.data_ptr() != self._span_words_ptr:
            raise RuntimeError("the GridSpan's occupancy grid's words tensor was replaced: its address is baked into the captured "
                               f"graph (TrainingOccupancyGrid.update writes in place); build a new {type(self).__name__}")

    def step(self, *args, **kw):
        self._watch_span()
        return super().step(*args, **kw)

    __call__ = step

    def _alloc_pass_buffers(self, tn, tf):
        super()._alloc_pass_buffers(tn, tf)
        ptr, first = _lib.ptr, self.passes[0]
        rays, jit, _, flags, seed, rid = first.jitter
        self.tbins01 = _tbins(0, 1, first.N, self.dev)
        self.ts_box = torch.empty((self.B, first.N), dtype=torch.float32, device=self.dev)
        self._box_jitter = (rays, jit, ptr(self.tbins01), flags, seed, rid)
        self._box_entry, args = self.box.placement(self.dev)
        self._box_args = (*args, *self._box_interval)
        first.jitter = (ptr(self.rays), ptr(self.ts_box), None, _lib.FLAG_TS_GIVEN, 0, 0)
        if not hasattr(self, "ts"):              # a masked pass keeps no positions of its own: the placed ones are the step's
            self.ts = self.ts_box

    def _before_forward(self, st):
        super()._before_forward(st)
        _launch(self._box_entry, *self._box_jitter, *self._box_args, self.ts_box, None, None, self.B, self.passes[0].N, st)


class GraphedBoxTrainStep(_BoxSteps, GraphedTrainStep):
    """``train_step(..., box=box)`` as captured hipGraphs: GraphedTrainStep with its one dense pass under
    NERF_AMD_TS_GIVEN and ONE more node in graph A:

        graph A: hyper fetch -> placement (nerf_amd_box_positions: the stepper's jitter on unit bins, each ray's interval
                 clipped to ``box``; writes ``ts_box`` [B, N]) -> training forward on ts_box -> head -> ...: the rest is
                 GraphedTrainStep's, and so are graph B, the exchange seam, ``rays_from``, ``controls`` and ``check_every``.

    Jitter and ``step`` as GraphedTrainStep; step k (1-based) equals the eager ``train_step(..., box=box, device_rng=True,
    seed=seed + k)``, or ``train_step(..., box=box, u=u)`` for a given ``u``.  ``stepper.ts`` holds the positions the forward
    read (the forward's own copy, bit for bit ``ts_box``).  The positions carry no gradient; the distortion term keeps the
    global ``tf``."""

    def __init__(self, net, optimizer, n_rays, N, box, *, tn=2, tf=6, **kw):
        self._bind_box(box, int(N), tn, tf)
        super().__init__(net, optimizer, n_rays, N, tn=tn, tf=tf, **kw)

    def _range_check(self):
        """The reference's |x| > 1 warning on the first / last PLACED position of every ray."""
        from .utils.xyz import range_check_rays
        range_check_rays(self.rays, self.ts_box, None, _lib.FLAG_TS_GIVEN, 0, 0, self.N)


class GraphedMaskedBoxTrainStep(_BoxSteps, GraphedMaskedTrainStep):
    """``train_step(..., occupancy=, box=box)`` as captured hipGraphs: GraphedMaskedTrainStep on the box's positions --

        graph A: hyper fetch -> placement (nerf_amd_box_positions; writes ``ts_box`` [B, N]) -> mark + scan, capped emit,
                 training forward on the C points and the masked head, all under NERF_AMD_TS_GIVEN on ts_box -> ...

    Capacity, overflow reporting, ``counts()``, ``rays_from``, ``controls`` and ``check_every`` are GraphedMaskedTrainStep's;
    with P' <= C step k equals the eager ``train_step(..., occupancy=, box=box, device_rng=True, seed=seed + k)``.  A tight box
    (``SceneBox.from_occupancy``) raises the live share of the batch: size the capacity for it."""

    def __init__(self, net, optimizer, n_rays, N, box, occupancy, capacity, *, tn=2, tf=6, **kw):
        self._bind_box(box, int(N), tn, tf)
        super().__init__(net, optimizer, n_rays, N, occupancy, capacity, tn=tn, tf=tf, **kw)


class _PairJitter:
    """The jitter of a stepper that draws coarse and fine positions (listed in front of its stepper base): ``u`` [B, Nc+Nf] of
    the reference stream as two views -- its first B*Nc values are torch.rand(B,Nc) = ``u_c``, the rest torch.rand(B,Nf) =
    ``u_f``, the same numbers as the two draws in a row -- and ``step(..., u_c=, u_f=)``."""

    def _split_u(self, Nc, Nf):
        flat_u, B = self.u.view(-1), self.B
        self.u_c, self.u_f = flat_u[:B * Nc].view(B, Nc), flat_u[B * Nc:].view(B, Nf)

    def step(self, rays=None, gt=None, u_c=None, u_f=None, decay=1.0):
        if (u_c is None) != (u_f is None):
            raise RuntimeError("step(): u_c and u_f come together (or neither)")
        u = None
        if u_c is not None:
            if tuple(u_c.shape) != tuple(self.u_c.shape) or tuple(u_f.shape) != tuple(self.u_f.shape):
                raise RuntimeError(f"u_c / u_f must be {tuple(self.u_c.shape)} / {tuple(self.u_f.shape)}")
            if self.device_rng:
                raise RuntimeError(f"this {type(self).__name__} draws its jitter on the device (device_rng=True): "
                                   "u_c / u_f must be None")
            self.u_c.copy_(u_c, non_blocking=True)
            self.u_f.copy_(u_f, non_blocking=True)
            u = self.u
        return super().step(rays, gt, u=u, decay=decay)

    __call__ = step


class GraphedHierarchicalTrainStep(_PairJitter, GraphedTrainStep):
    """``train_step_hierarchical`` for the fused bf16 path as captured hipGraphs: GraphedTrainStep with two dense passes,
    coarse and fine (hyper ring, status watch, ``rays_from`` selection in both jitter modes, exchange, capture: inherited):

        graph A: hyper fetch -> coarse training forward (Nc stratified samples) -> coarse head (compositor + MSE gradient
                 + compositor backward + sample_pdf on the coarse weights, ONE kernel:
                 nerf_amd_volume_render_mse_backward_pdf, writes ts_f) -> fine training forward on ts_f (Nc+Nf samples,
                 NERF_AMD_TS_GIVEN) -> fine compositor + MSE gradient + backward -> both dX chains -> both sets of dW
                 products into ONE combined gradient vector (coarse first, the optimizer's order); GraphedTrainStep's side
                 branch with both passes' launches and the sum of the two loss values on it
        graph B: one Adam launch over both networks' flat vector -> re-pack of both networks' training images

    ``optimizer`` must be ``optim.FusedAdam([net_c, net_f])``.  Jitter as in GraphedTrainStep: default the reference-style
    CPU draws torch.rand(B,Nc) then torch.rand(B,Nf) (one draw of B*(Nc+Nf) from the same stream, continued on the
    device); ``device_rng=True`` keys both draws by seed + step (the eager step's values with ``seed=seed + k`` at step k).
    ``step(rays=None, gt=None, u_c=None, u_f=None, decay=1.0)`` returns the total loss as a 0-d device tensor (no sync);
    ``losses`` holds [coarse, fine]; ``net_c`` / ``net_f`` are the two modules, ``net`` = ``nets`` the pair (as
    ``FusedAdam([net_c, net_f]).net``).  bf16 storage, one exchange bucket.

    ``controls``: a ``Controls`` with a background and / or sigma noise -- the coarse head becomes
    nerf_amd_volume_render_mse_backward_pdf_bg and the fine head nerf_amd_volume_render_mse_backward_bg: the same number of
    launches.  ``stepper.background`` is the stepper's own buffer (one colour or [n_rays, 3]), overwritable in place between
    replays; ``stepper.sigma_noise`` is read-only.  Step k (1-based) draws the coarse noise under ``noise_seed + k`` and the
    fine noise under ``noise_seed + FINE_NOISE_OFFSET + k``, both with the stepper's ``ray_id0``: the eager
    ``train_step_hierarchical(..., seed=seed + k, controls=controls.replace(noise_seed=noise_seed + k))``.
    ``controls.distortion > 0`` raises RuntimeError before anything else is looked at; the flat ``distortion=`` keyword keeps
    its refusal.  Without ``controls`` the step is the one it was, launch for launch."""

    _one_bucket = True

    def __init__(self, net_c, net_f, optimizer, n_rays, Nc=64, Nf=128, *, tn=2, tf=6, group=None, device_rng=False, seed=0,
                 ray_id0=0, check_every=16, rays_from=None, select_mode="train", distortion=0.0, controls=None):
        c = controls_mod.pair(controls, type(self).__name__)
        controls_mod.check_distortion(distortion, {"a coarse / fine pair": (net_c, net_f)})
        _check_pair(net_c, net_f, Nc, Nf, None)
        self.net_c, self.net_f, self.Nc, self.Nf = net_c, net_f, int(Nc), int(Nf)
        # ``net`` / ``nets`` are the pair, as FusedAdam([net_c, net_f]).net / .nets hold it
        self.nets = (net_c, net_f)
        self._samples = (self.Nc, self.Nc + self.Nf)
        super().__init__(self.nets, optimizer, n_rays, self.Nc + self.Nf, tn=tn, tf=tf, group=group, device_rng=device_rng,
                         seed=seed, ray_id0=ray_id0, check_every=check_every, rays_from=rays_from, select_mode=select_mode,
                         **({} if c is None else {"controls": c}))

    def _check_modules(self, net, optimizer):
        from .optim import FusedAdam
        if not isinstance(optimizer, FusedAdam):
            raise RuntimeError("GraphedHierarchicalTrainStep needs optim.FusedAdam([net_c, net_f])")
        if optimizer.nets is None or len(optimizer.nets) != 2 or optimizer.nets[0] is not net[0] or optimizer.nets[1] is not net[1]:
            raise RuntimeError("the optimizer is not FusedAdam([net_c, net_f]) of this pair")
        _check_fused_trainable(net[0].precision)

class GraphedMaskedHierarchicalTrainStep(_MaskedSteps, GraphedHierarchicalTrainStep):
    """``train_step_hierarchical(..., occupancy=)`` as captured hipGraphs: GraphedHierarchicalTrainStep's
    pair (one FusedAdam([net_c, net_f]), one combined gradient vector, the ``u_c`` / ``u_f`` jitter) with each pass run as
    GraphedMaskedTrainStep runs its one -- on a fixed point capacity, the live counts never reaching the host.

        graph A: hyper fetch -> mark + scan (coarse jitter) -> capped emit (C_c points) -> coarse training forward on them
                 -> masked coarse head (masked compositor + MSE gradient + backward + sample_pdf on its weights, ONE kernel:
                 nerf_amd_volume_render_masked_mse_backward_pdf, writes ts_f) -> mark + scan with NERF_AMD_TS_GIVEN on ts_f
                 -> capped emit (C_f points) -> fine training forward -> fused masked head (NERF_AMD_TS_GIVEN) -> both dX
                 chains -> both sets of dW products into the combined gradient vector, coarse first; the side branch as
                 GraphedHierarchicalTrainStep's
        graph B and the all-reduce seam: inherited (one exchange bucket; ``group`` is handed through unchanged).

    ``capacity`` = (C_c, C_f): each an int (points) or a float (fraction of n_rays * Nc, of n_rays * (Nc + Nf)); NO default.
    The fine samples gather where the coarse weights are, so the fine pass's live fraction is not the coarse pass's.
    An overflow of either pass treats that pass's tail of live samples (ray-major) as dead, exactly as GraphedMaskedTrainStep:
    with C_c short the sampler sees weights under the stricter mask.  Device ``counts``: int64[4] = {P'_c, kept_c, P'_f,
    kept_f}; every ``check_every`` steps they are copied back without waiting: ``last_stats`` = {'step', 'coarse': {...},
    'fine': {...}} (each {'samples', 'live', 'kept', 'capacity'}), an observed overflow raises a RuntimeWarning naming the
    pass (``overflow_steps`` counts steps), ``counts()`` reads the latest step's now (one sync).

    ``occupancy``: ONE grid for both passes; its ``words`` address is baked into the graph (``step`` raises if the tensor was
    replaced; an in-place ``TrainingOccupancyGrid.update(net_f, ...)`` takes effect on the next replay).  ``losses`` holds
    [coarse, fine].  bf16 storage, the default network, 3 <= Nc <= 256, Nc + Nf <= 512.

    ``controls``: as GraphedHierarchicalTrainStep's -- the masked coarse head becomes
    nerf_amd_volume_render_masked_mse_backward_pdf_bg (the sampler sees the weights of the noisy masked compositor under the
    clamp) and the fine head nerf_amd_volume_render_masked_mse_backward_dist with the distortion term's scalars zero."""

    def __init__(self, net_c, net_f, optimizer, n_rays, Nc, Nf, occupancy, capacity, *, tn=2, tf=6, group=None, device_rng=False,
                 seed=0, ray_id0=0, check_every=16, rays_from=None, select_mode="train", buckets=1, storage="bf16",
                 distortion=0.0, controls=None):
        controls_mod.pair(controls, type(self).__name__)
        controls_mod.check_distortion(distortion, {"an occupancy grid": occupancy})
        self._refuse(storage, buckets)
        _check_pair(net_c, net_f, Nc, Nf, None)
        B, Nc_, Nf_ = int(n_rays), int(Nc), int(Nf)
        if B < 1:
            raise ValueError(f"{type(self).__name__} needs n_rays >= 1 (got {n_rays})")
        self._bind_grid((net_c, net_f), (Nc_, Nc_ + Nf_), B, optimizer, occupancy, capacity)
        self.capacity = self._capacities
        super().__init__(net_c, net_f, optimizer, B, Nc_, Nf_, tn=tn, tf=tf, group=group, device_rng=device_rng, seed=seed,
                         ray_id0=ray_id0, check_every=check_every, rays_from=rays_from, select_mode=select_mode,
                         controls=controls)

    def step(self, rays=None, gt=None, u_c=None, u_f=None, decay=1.0):
        self._watch_grid()
        return super().step(rays, gt, u_c=u_c, u_f=u_f, decay=decay)

    __call__ = step


class GraphedGuidedTrainStep(_PairJitter, GraphedTrainStep):
    """``train_step_guided`` as captured hipGraphs: GraphedTrainStep with its one dense pass at
    N = Nc + Nf under NERF_AMD_TS_GIVEN, and ONE more node in graph A:

        graph A: hyper fetch -> guided sampler (nerf_amd_sample_pdf_volume: coarse positions, look-up in the proposal's sigma
                 volume, weights, sample_pdf; writes ``ts_f`` [B, Nc+Nf]) -> training forward on ts_f -> head -> ...: the rest
                 is GraphedTrainStep's, and so are graph B, the exchange seam, ``rays_from`` and ``check_every``.

    ``proposal``: a ``ProposalVolume`` on the module's device.  The address of its ``sigma`` is baked into the graph (``step``
    raises if the tensor was replaced); ``ProposalVolume.update`` writes in place, so an update between two replays simply
    takes effect.  Jitter: default the reference-style CPU draws torch.rand(B,Nc) then torch.rand(B,Nf) (one draw of
    B*(Nc+Nf) from the same stream, continued on the device), or ``step(..., u_c=, u_f=)``; ``device_rng=True`` keys both draws
    by seed + step, read from device memory (the eager step's values with ``seed=seed + k`` at step k).
    ``optimizer`` is ``optim.FusedAdam(net)``: one network, one Adam launch.  bf16 storage, one exchange bucket."""

    _one_bucket = True

    def __init__(self, net, optimizer, n_rays, Nc, Nf, proposal, *, tn=2, tf=6, group=None, device_rng=False, seed=0,
                 ray_id0=0, check_every=16, rays_from=None, select_mode="train", buckets=1, storage="bf16", distortion=0.0,
                 controls=None):
        from .utils.proposal import check_sizes
        lam = controls_mod.check_distortion(distortion, {"an occupancy grid": self._capacities})   # the masked guided stepper too
        controls = controls_mod.bundle(controls, distortion=distortion)
        if controls is not None and self._capacities is None and (controls.background is not None or controls.sigma_noise):
            raise RuntimeError("the dense guided stepper takes the distortion term only: background / sigma_noise need the "
                               "masked guided stepper (GraphedMaskedGuidedTrainStep)")
        _MaskedSteps._refuse(self, storage, buckets)
        _check_guided(net, proposal)
        self.Nc, self.Nf = check_sizes(Nc, Nf)
        if int(n_rays) < 1:
            raise ValueError(f"GraphedGuidedTrainStep needs n_rays >= 1 (got {n_rays})")
        self._check_modules(net, optimizer)
        if proposal.sigma.device != optimizer.flat.device:
            raise RuntimeError(f"the proposal volume lives on {proposal.sigma.device}, the module on {optimizer.flat.device}")
        proposal.check(torch.empty((0, 6), dtype=torch.float32, device=proposal.sigma.device), self.Nc, self.Nf)
        self.proposal, self._sigma_ptr = proposal, proposal.sigma.data_ptr()
        super().__init__(net, optimizer, n_rays, self.Nc + self.Nf, tn=tn, tf=tf, group=group, device_rng=device_rng, seed=seed,
                         ray_id0=ray_id0, check_every=check_every, rays_from=rays_from, select_mode=select_mode, distortion=lam,
                         controls=controls)

    def _alloc_pass_buffers(self, tn, tf):
        """The dense pass reads given positions: ``ts_f``, which the sampler writes.  ``u`` is split as a pair's."""
        super()._alloc_pass_buffers(tn, tf)
        ptr, B, Nc, Nf, dev = _lib.ptr, self.B, self.Nc, self.Nf, self.dev
        self.tbins = _tbins(tn, tf, Nc, dev)                        # of the COARSE positions, the only ones drawn from bins
        self._split_u(Nc, Nf)
        self.ts_f = torch.empty((B, Nc + Nf), dtype=torch.float32, device=dev)
        if self.device_rng:
            self._coarse_jitter = (ptr(self.rays), self._seed_mem, ptr(self.tbins),
                                   _lib.FLAG_DEVICE_RNG | _lib.FLAG_SEED_IN_MEMORY, self.seed, self.ray_id0)
        else:
            self._coarse_jitter = (ptr(self.rays), ptr(self.u_c), ptr(self.tbins), 0, 0, 0)
        self.passes[0].jitter = (ptr(self.rays), ptr(self.ts_f), None, _lib.FLAG_TS_GIVEN, 0, 0)

    def _before_forward(self, st):
        p = self.proposal
        _launch("nerf_amd_sample_pdf_volume", *self._coarse_jitter, self._sigma_ptr, *p.resolution, p._h_lo,
                p._h_inv_step, None if self.device_rng else self.u_f, self.ts_f, None, None, self.B, self.Nc, self.Nf, st)

    def _range_check(self):
        """The reference's |x| > 1 warning on the coarse positions' first / last samples (the new ones lie between)."""
        from .utils.xyz import range_check_rays
        _, jit, _, flags, seed, rid = self._coarse_jitter
        range_check_rays(self.rays, jit, self.tbins, flags, seed, rid, self.Nc)

    def step(self, rays=None, gt=None, u_c=None, u_f=None, decay=1.0):
        if self.proposal.sigma.data_ptr() != self._sigma_ptr:
            raise RuntimeError("the proposal's sigma tensor was replaced: its address is baked into the captured graph "
                               "(ProposalVolume.update writes in place); build a new GraphedGuidedTrainStep")
        return super().step(rays, gt, u_c=u_c, u_f=u_f, decay=decay)

    __call__ = step


class GraphedMaskedGuidedTrainStep(_MaskedSteps, GraphedGuidedTrainStep):
    """``train_step_guided(..., occupancy=)`` as captured hipGraphs: GraphedGuidedTrainStep with its one
    pass masked on a fixed point capacity, as GraphedMaskedTrainStep runs its one -- the cheapest step this package has: one
    network, its samples gathered where the volume says the surface is, empty space never evaluated.

        graph A: hyper fetch -> masked guided placement (nerf_amd_sample_pdf_volume_masked: coarse positions, look-up in the
                 proposal's sigma volume, dead coarse samples weighed 0, sample_pdf, mark + scan of the merged positions; writes
                 ``ts_f`` [B, Nc+Nf], ``mask``, ``offsets``) -> capped emit on ts_f (nerf_amd_occupancy_points_capped: pts[C, 6],
                 counts) -> training forward on the C points -> masked head (nerf_amd_volume_render_masked_mse_backward under
                 NERF_AMD_TS_GIVEN) -> dX chain -> dW products; the side branch beside the dX chain is GraphedTrainStep's.
                 nerf_amd_occupancy_mark is not launched: the placement marks what it places.
        graph B and the all-reduce seam: GraphedTrainStep's, unchanged (one exchange bucket).

    ``capacity``: points, or a fraction of n_rays * (Nc + Nf); NO default.  Overflow, ``counts()``, ``last_stats``,
    ``overflow_steps`` and the RuntimeWarning are GraphedMaskedTrainStep's; jitter, ``step(rays, gt, u_c=, u_f=)`` and
    ``rays_from`` are GraphedGuidedTrainStep's.  The addresses of ``occupancy.words`` and ``proposal.sigma`` are baked into
    the graph (``step`` raises if either tensor was replaced); ``TrainingOccupancyGrid.update`` and ``ProposalVolume.update``
    write in place, so an update between two replays simply takes effect.  With P' <= C at step k the step is the eager
    ``train_step_guided(..., occupancy=, device_rng=True, seed=seed + k)``.  bf16 storage, the default network.
    ``controls``: GraphedMaskedTrainStep's -- the same head with the three terms on the Nc + Nf guided positions; the eager
    equivalent at step k is ``train_step_guided(..., occupancy=, controls=c.replace(noise_seed=c.noise_seed + k))``."""

    _masked_pass_type = _MarkedPass

    def __init__(self, net, optimizer, n_rays, Nc, Nf, proposal, occupancy, capacity, *, tn=2, tf=6, group=None, device_rng=False,
                 seed=0, ray_id0=0, check_every=16, rays_from=None, select_mode="train", buckets=1, storage="bf16",
                 distortion=0.0, controls=None):
        from .utils.proposal import check_sizes
        controls_mod.check_distortion(distortion, {"an occupancy grid": occupancy})
        controls = controls_mod.bundle(controls)
        self._refuse(storage, buckets)
        _check_guided(net, proposal)
        Nc_, Nf_ = check_sizes(Nc, Nf)
        B = int(n_rays)
        if B < 1:
            raise ValueError(f"{type(self).__name__} needs n_rays >= 1 (got {n_rays})")
        self._bind_grid((net,), (Nc_ + Nf_,), B, optimizer, occupancy, capacity)
        self.capacity = self._capacities[0]
        super().__init__(net, optimizer, B, Nc_, Nf_, proposal, tn=tn, tf=tf, group=group, device_rng=device_rng, seed=seed,
                         ray_id0=ray_id0, check_every=check_every, rays_from=rays_from, select_mode=select_mode, controls=controls)

    def _before_forward(self, st):
        p, m = self.proposal, self.passes[0]
        R, lo, inv, outside = self._grid
        rays, jit, tbins, flags, seed, rid = self._coarse_jitter
        _launch("nerf_amd_sample_pdf_volume_masked", rays, jit, tbins, flags | outside, seed, rid,
                self._sigma_ptr, *p.resolution, p._h_lo, p._h_inv_step, self._words_ptr, *R, lo,
                inv, None if self.device_rng else self.u_f, self.ts_f, None, None, m.mask, m.offsets, None,
                self._mark_ws, self.B, self.Nc, self.Nf, st)

    def step(self, rays=None, gt=None, u_c=None, u_f=None, decay=1.0):
        self._watch_grid()
        return super().step(rays, gt, u_c=u_c, u_f=u_f, decay=decay)

    __call__ = step
