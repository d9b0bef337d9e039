"""CPU model of the per-image colour correction (test infrastructure; uses the oracle): csrc/appearance_device.h, the four
stages of csrc/appearance.hip and the float64 value of the head that carries the map (nerf_amd_volume_render_mse_backward_affine).
Imports oracle.nerf_oracle, tests/ray_routines_model.py and tests/input_grad_model.py and edits none of them.

The map.  Image m holds theta[m] = (a[3], b[3]); a ray of it sees  c' = (1 + a) * c + b  -- ``apply`` below, three separately
rounded torch ops per channel in the tensors' dtype: in fp32 this IS the kernels' definition (compared with torch.equal), in
float64 the truth.  Its backward, each one product: g_c = g (1 + a), the ray's row of g_theta = (g c, g).  The image of a ray
is id // HW; an id outside [0, M HW) has a row of NaN and reaches no image.

The reduction.  g_theta[m] = sum of the rows of image m (+ reg theta[m]; a frozen image: exactly 0).  A sum of n fp32 terms in
ANY fixed order lies within (n - 1) EPS sum |x| of the exact sum to first order (every partial sum is bounded by sum |x| and
every one of the n - 1 additions rounds once, EPS = 2^-24 relative).  The ridge adds one term that is itself one rounded
product: n additions on sum |x| + |reg theta|, plus EPS |reg theta|.  ``reduce64`` returns the float64 value and that bound.

Head against float64.  loss = MSE(c', gt): its gradient with respect to raw is the compositor's backward with the upstream
g_rgb = (1 + a) 2 (c' - gt) / (3 B) formed from the float64 forward; ray_routines_model.model_backward gives the value and the
first-order bound A, ray_routines_model.ray_ratios the two ratios per ray.  As in tests/background_model.py the upstream is
formed from the forward in fp32 as well, so it has constants of its own, C_REF_APP / C_REF_APP_PLAIN: the largest ratio of the
reference's own fp32 evaluation (oracle.volume_render + the map + MSE under fp32 autograd) over head_cases().  The cases are
the raw outputs of the `structured` synthetic weights and of their high-gain form (first layer x 1e5, second / 1e5) on 37 rays
at N in {2, 64, 65, 192} (N = 1, the reference's empty sample axis, has no sample to judge: the GPU test states it in closed
form).  RECOVERY_F_FIXED / RECOVERY_F_FRESH: the factor by which the fp32 CPU loop cuts ||theta - theta*|| on recovery_scene()
with fixed jitter and with a fresh draw per step.  All of them are written by

    python tests/appearance_model.py            (a few minutes on a CPU; prints the four constants)

the C_REF pair rounded up to two digits, the recovery factors rounded down; tests/test_appearance_cpu.py asserts that the
oracle's fp32 evaluation stays inside them, and the GPU test allows the model's usual  bound(c) = 2 c + 4.  Nothing here is
taken from what a GPU shows.
"""
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "oracle"), os.path.join(_ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import nerf_oracle as O  # noqa: E402
import input_grad_model as IG  # noqa: E402
import ray_routines_model as M  # noqa: E402

EPS = M.EPS

# measured on the CPU by `python tests/appearance_model.py` (see the module docstring)
C_REF_APP = 3.6
C_REF_APP_PLAIN = 18.0
RECOVERY_F_FIXED = 7.8           # measured 7.871, rounded down to two digits
RECOVERY_F_FRESH = 7.0           # measured 7.094


# ---- the map ------------------------------------------------------------------------------------------------------------------
def apply(rgb, rows):
    """rgb [B,3], rows [B,6] or [6] -> c': (1 + a) * c + b in the tensors' dtype, every op rounded on its own."""
    return (1 + rows[..., :3]) * rgb + rows[..., 3:]


def apply_backward(g, rgb, rows):
    """g [B,3] = d loss / d c' -> (g_rgb [B,3], g_theta_ray [B,6] = (g c, g))."""
    return g * (1 + rows[..., :3]), torch.cat([g * rgb, g.expand_as(rgb)], dim=-1)


def valid_rows(ids, M_, HW):
    return (ids >= 0) & (ids < M_ * HW)


def gather(theta, ids, HW):
    """theta [M,6], ids [B] -> rows [B,6]; NaN for an id outside [0, M HW)."""
    ok = valid_rows(ids, theta.shape[0], HW)
    rows = torch.full((ids.shape[0], 6), float("nan"), dtype=theta.dtype)
    rows[ok] = theta[torch.div(ids[ok], HW, rounding_mode="floor")]
    return rows


def mse_gradient(pred, target):
    """The MSE head's g = 2 (pred - target) / (3 B) as the kernels form it (csrc/composite_backward_device.h)."""
    B = pred.shape[0]
    scale = (torch.tensor(1.0) / (torch.tensor(3.0) * torch.tensor(float(B)))).to(pred.device)
    return 2.0 * (pred - target) * scale


def reduce64(g_ray, ids, HW, theta, reg=0.0, frozen=()):
    """(want [M,6] float64, bound [M,6]) of nerf_amd_appearance_reduce on the fp32 rows ``g_ray``: see the module docstring."""
    M_ = theta.shape[0]
    want, bound = np.zeros((M_, 6)), np.zeros((M_, 6))
    g, th = g_ray.double().numpy(), theta.double().numpy()
    img = torch.div(ids, HW, rounding_mode="floor").numpy()
    ok = valid_rows(ids, M_, HW).numpy()
    for m in range(M_):
        if m in frozen:
            continue
        rows = g[ok & (img == m)]
        ridge = float(np.float32(reg)) * th[m]
        want[m] = rows.sum(axis=0) + ridge
        if reg:         # n + 1 terms, the last one a rounded product
            bound[m] = len(rows) * EPS * (np.abs(rows).sum(axis=0) + np.abs(ridge)) + EPS * np.abs(ridge)
        else:           # the ridge term is an exact zero: n terms, n - 1 additions
            bound[m] = max(len(rows) - 1, 0) * EPS * np.abs(rows).sum(axis=0)
    return want, bound


# ---- the head's cases ---------------------------------------------------------------------------------------------------------
HEAD_N = (2, 64, 65, 192)
HEAD_B, HEAD_M, HEAD_HW = 37, 4, 16
HEAD_KINDS = ("structured", "high_gain")


def high_gain_state_dict(gain=1e5):
    """The structured weights with the first hidden layer scaled up by ``gain`` and the second layer's weights scaled down by
    it (tests/test_gpu_boundary.py): the same function in exact arithmetic, first activations ``gain`` times larger."""
    from nerf_simple_amd.utils import synthetic
    sd = {k: v.clone() for k, v in synthetic.synthetic_state_dict(0, "structured").items()}
    sd["layers_0.0.weight"] *= gain
    sd["layers_0.0.bias"] *= gain
    sd["layers_0.2.weight"] /= gain
    return sd


def head_cases():
    return [(kind, N) for kind in HEAD_KINDS for N in HEAD_N]


_RAW = {}


def head_inputs(kind, N):
    """raw [37,N,4] (the fp32 oracle's network output on the weights of ``kind``), ts, rays, target [37,3], theta [4,6],
    ids [37] (repeats, every id valid).  N == 1 is served too (the GPU test's closed form needs the inputs)."""
    if (kind, N) not in _RAW:
        from nerf_simple_amd.utils import synthetic
        sd = synthetic.synthetic_state_dict(0, "structured") if kind == "structured" else high_gain_state_dict()
        g = torch.Generator().manual_seed(700 + N + (1000 if kind != "structured" else 0))
        pose = torch.from_numpy(O.spherical_to_pose(4, -30, 0)).float()
        table = O.camera_rays(pose, [8, 8, synthetic.focal_from_fov(8)])
        rays = table[torch.randperm(64, generator=g)[:HEAD_B]].contiguous()
        ts = O.sample_ts(torch.rand(HEAD_B, N, generator=g))
        with torch.no_grad():
            q, _ = O.query_points(rays, ts)
            raw = O.nerf_forward(sd, q).reshape(HEAD_B, N, 4).contiguous()
        target = torch.rand(HEAD_B, 3, generator=g)
        theta = torch.cat([torch.rand(HEAD_M, 3, generator=g) * 0.6 - 0.3, torch.rand(HEAD_M, 3, generator=g) * 0.1 - 0.05], dim=1)
        ids = torch.randint(0, HEAD_M * HEAD_HW, (HEAD_B,), generator=g)
        _RAW[(kind, N)] = (raw, ts, rays, target, theta, ids)
    return _RAW[(kind, N)]


def unit_dirs(rays):
    d = rays[:, 3:]
    return d / torch.norm(d, dim=1, keepdim=True)


def head_model(raw, ts, rays, target, rows):
    """float64 (want [B,N,4], A [B,N,4], c' [B,3], g_theta_ray [B,6], rgb [B,3]) of d MSE((1 + a) rgb + b, target) / d raw."""
    fw = M.forward64(raw, ts, unit_dirs(rays))
    B = ts.shape[0]
    rgb = (fw["w"][..., None] * raw[..., :3].double()).sum(dim=1)
    r64 = rows.double()
    pred = apply(rgb, r64)
    g = 2.0 * (pred - target.double()) / (3.0 * B)
    g_rgb, g_ray = apply_backward(g, rgb, r64)
    want, A = M.model_backward(fw, raw, ts, [g_rgb, None, None, None, None])
    return want, A, pred.numpy(), g_ray.numpy(), rgb.numpy()


def oracle_head_grad(raw, ts, rays, target, rows, dtype):
    """The same gradients through the oracle's autograd in ``dtype`` (the reference's own evaluation): (d_raw, g_theta_ray)."""
    r = raw.to(dtype).clone().requires_grad_(True)
    th = rows.to(dtype).clone().requires_grad_(True)
    rgb = O.volume_render(r, ts.to(dtype), unit_dirs(rays).to(dtype))[0]
    torch.mean((apply(rgb, th) - target.to(dtype)) ** 2).backward()
    return r.grad.double().numpy(), th.grad.double().numpy()


def measure():
    c_cond = c_plain = 0.0
    for kind, N in head_cases():
        raw, ts, rays, target, theta, ids = head_inputs(kind, N)
        rows = gather(theta, ids, HEAD_HW)
        want, A = head_model(raw, ts, rays, target, rows)[:2]
        ref32, _ = oracle_head_grad(raw, ts, rays, target, rows, torch.float32)
        cond, plain = M.ray_ratios(ref32, want, A, np.isfinite(ref32))
        c_cond, c_plain = max(c_cond, float(cond.max())), max(c_plain, float(np.nanmax(plain, initial=0.0)))
    return c_cond, c_plain


# ---- recovery of known corrections over three images ------------------------------------------------------------------------------
REC_SIDE, REC_N, REC_LR, REC_STEPS, REC_LEVELS = 12, 32, 0.02, 40, 3
REC_HW = REC_SIDE * REC_SIDE
REC_POSES = ((4, -30, 0), (4, -45, 120), (4, -20, 240))           # spherical (r, theta deg, phi deg)
REC_FROZEN = (0,)


def recovery_truth():
    """theta* [3,6] fp32: image 0 at the identity (it is the frozen anchor), gains in [0.7, 1.3], biases within +-0.05."""
    g = torch.Generator().manual_seed(11)
    th = torch.cat([torch.rand(3, 3, generator=g) * 0.6 - 0.3, torch.rand(3, 3, generator=g) * 0.1 - 0.05], dim=1)
    th[0] = 0
    return th.contiguous()


def recovery_error(theta):
    return float((theta.detach().double().cpu() - recovery_truth().double()).norm())


def recovery_scene():
    """(smooth state dict, stored poses [3,4,4] fp32, cam_params) of the three-image scene."""
    from nerf_simple_amd.utils import synthetic
    sd = IG.smooth_state_dict(synthetic.synthetic_state_dict(0, "structured"), REC_LEVELS)
    poses = torch.stack([torch.from_numpy(O.spherical_to_pose(*p)).float() for p in REC_POSES])
    return sd, poses, [REC_SIDE, REC_SIDE, synthetic.focal_from_fov(REC_SIDE)]


def recovery_jitter():
    return torch.rand(3 * REC_HW, REC_N, generator=torch.Generator().manual_seed(0))


def recovery_target(rgb):
    """The colours of the scene's pixels: the frozen net's own render ``rgb`` [3 HW, 3] (image by image) through theta*."""
    return apply(rgb, recovery_truth().to(rgb.device).repeat_interleave(REC_HW, dim=0))


def oracle_recovery(fresh):
    """The factor by which REC_STEPS Adam steps (lr REC_LR) on the fp32 CPU oracle cut ||theta - theta*||: all 3 x 12 x 12 rays
    per step, theta from zero, image 0 held."""
    sd, poses, cam = recovery_scene()
    rays = torch.cat([O.camera_rays(p, cam) for p in poses])
    ids = torch.arange(3 * REC_HW)
    g = torch.Generator().manual_seed(1)
    u = recovery_jitter()
    with torch.no_grad():
        rgb = IG.render(IG.exact_forward, sd, rays, REC_N, u=u)[0]
        target = recovery_target(rgb)
    theta = torch.zeros(3, 6, requires_grad=True)
    opt = torch.optim.Adam([theta], lr=REC_LR)
    e0 = recovery_error(theta)
    for _ in range(REC_STEPS):
        if fresh:
            with torch.no_grad():
                rgb = IG.render(IG.exact_forward, sd, rays, REC_N, u=torch.rand(len(ids), REC_N, generator=g))[0]
        opt.zero_grad()
        torch.nn.functional.mse_loss(apply(rgb, gather(theta, ids, REC_HW)), target).backward()
        theta.grad[list(REC_FROZEN)] = 0
        opt.step()
    return e0 / recovery_error(theta)


if __name__ == "__main__":
    print("C_REF_APP = %.3g   C_REF_APP_PLAIN = %.3g" % measure())
    print("RECOVERY_F_FIXED = %.4g   RECOVERY_F_FRESH = %.4g" % (oracle_recovery(False), oracle_recovery(True)))
