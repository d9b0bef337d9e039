"""Float64 model of the camera optimiser's kernels (test infrastructure): tests/input_grad_model.pose_rays over M images.

Definition (include/nerf_amd.h, restated).  Image m of M has the stored pose [R0 | t0] (fp32) and the correction
xi[m] = (w, tau) (fp32): R = exp([w]x) R0, t = t0 + tau.  The global ray id r = m H W + h W + w names the ray
[t, R dir_cam], dir_cam = ((w - W//2)/f, -(h - H//2)/f, -1) with f the fp32 focal length.  ``rays`` below evaluates exactly
input_grad_model.pose_rays per image (torch.linalg.matrix_exp of the skew matrix), in the dtype it is given; the gradient
of sum(rays * d_rays) with respect to xi is torch autograd through it.  An id outside [0, M H W) is a NaN row and takes
no part in any gradient.

The backward kernel does not differentiate the exponential: it uses g_w = J^T sum_rows (y x g_d), y = R dir_cam and
J = I + b K + c K^2 the left Jacobian of SO(3) (b = (1 - cos theta)/theta^2, c = (theta - sin theta)/theta^3).
``identity_grad`` is that expression in float64; tests/test_camera_cpu.py holds it against the autograd at every THETA.

Units (functions of the float64 intermediates only; EPS = 2^-24):
    direction component k of a row:   EPS sum_j |R_kj| |d_j|
      ... conditioned:                EPS sum_j (|exp([w]x)| |R0|)_kj |d_j|
    origin component k:               EPS (|t0_k| + |tau_k|)
    g_w of image m (each component):  EPS sum_rows |y| |g_d|           (Euclidean norms)
    g_tau of image m, component k:    EPS sum_rows |g_o,k|
A value whose unit is 0 must be met exactly (an image without a row: zeros).  The first direction unit takes the entries
of R as exact to a relative rounding; where the product exp([w]x) R0 cancels (an entry of R near 0 seen by a pixel near the
optical axis) any fp32 evaluation, torch's included, sits thousands of such units away, and the constant measured in it is
accordingly large.  The conditioned unit is what one rounding of every product in exp([w]x) R0 dir_cam costs; both are judged.

Constants C_REF_CAM_*: the largest ratio |fp32 - float64| / unit of torch's OWN fp32 evaluation of the same expression
(pose_rays in fp32 and its fp32 autograd) over cases() x THETAS, written by

    python tests/camera_model.py            (seconds on a CPU; prints the constants)

rounded up to two digits.  tests/test_camera_cpu.py asserts that the fp32 reference stays inside them and reaches half of
them; the kernels are allowed ray_routines_model.bound(c) = 2 c + 4.  Nothing here is taken from what a GPU shows.

Pose recovery (tests/test_gpu_camera.py; the scene of test_gpu_input_gradients.test_pose_recovery over three images).  The
same loops on the fp32 CPU oracle, run by `python tests/camera_model.py recovery` (minutes), cut the summed pose error by
    RECOVERY_F_FIXED   with the jitter fixed over the 30 steps           (eager test: the GPU must reach F / 1.8)
    RECOVERY_F_FRESH   with a fresh torch.rand jitter draw per step      (graphed test: the GPU must reach F / 2)
"""
import math
import os
import sys
from collections import namedtuple

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "oracle"), os.path.join(_ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import input_grad_model as IG  # noqa: E402
import ray_routines_model as RM  # noqa: E402

EPS = RM.EPS
bound = RM.bound

# measured on the CPU by `python tests/camera_model.py` (see the module docstring)
C_REF_CAM_DIR = 3600.0
C_REF_CAM_ORIGIN = 0.97
C_REF_CAM_GW = 12.0
C_REF_CAM_GTAU = 1.5
C_REF_CAM_DIR_COND = 410.0
# measured on the CPU by `python tests/camera_model.py recovery`
RECOVERY_F_FIXED = 4.57
RECOVERY_F_FRESH = 3.78         # N = 32 descends (N = 64: 4.46, N = 128: 4.52): N stays 32
RECOVERY_N_FRESH = 32            # samples per ray of the fresh-jitter loop (raised until the oracle descends)

H, W, F = 5, 7, 6.5              # non-square, odd
TAYLOR_BELOW = 1.0               # csrc/camera_device.h: on theta^2
THETAS = (0.0, 1e-6, 1e-3, 0.999, 1.001, 0.1, 0.5, 1.0, 3.0)
CAM_M = (1, 3, 70)
CAM_B = (1, 63, 64, 65, 257, 1000)
KINDS = ("mixed", "one_image", "ends")

CamCase = namedtuple("CamCase", "id M B kind seed")


def cases():
    out = []
    for M in CAM_M:
        for B in CAM_B:
            for kind in KINDS:
                out.append(CamCase(f"M{M}-B{B}-{kind}", M, B, kind, 9000 + len(out)))
    return out


def stored_poses(M, seed):
    """[M,3,4] fp32: a random rotation (QR of a Gaussian matrix, det +1) and a camera centre at radius 4."""
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(M, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2))[:, None, :]
    q[:, :, 0] *= torch.det(q)[:, None]
    c = torch.randn(M, 3, generator=g, dtype=torch.float64)
    c = 4.0 * c / c.norm(dim=1, keepdim=True)
    return torch.cat([q, c[:, :, None]], dim=2).float().contiguous()


def corrections(M, theta, seed):
    """xi [M,6] fp32: |w| = theta about a random axis per image, tau of a few hundredths."""
    g = torch.Generator().manual_seed(seed + 1)
    axis = torch.randn(M, 3, generator=g, dtype=torch.float64)
    axis = axis / axis.norm(dim=1, keepdim=True)
    tau = 0.05 * torch.randn(M, 3, generator=g, dtype=torch.float64)
    return torch.cat([axis * theta, tau], dim=1).float().contiguous()


def ray_ids(case):
    """ids [B] int64 in random order with duplicates.  'mixed': any image, and (B >= 3) one id = M H W and one = -1;
    'one_image': every row from one image; 'ends': images 0 and M - 1 only."""
    g = torch.Generator().manual_seed(case.seed + 2)
    HW = H * W
    pix = torch.randint(0, HW, (case.B,), generator=g)
    if case.kind == "mixed":
        img = torch.randint(0, case.M, (case.B,), generator=g)
    elif case.kind == "one_image":
        img = torch.full((case.B,), int(torch.randint(0, case.M, (1,), generator=g)))
    else:
        img = torch.randint(0, 2, (case.B,), generator=g) * (case.M - 1)
    ids = img * HW + pix
    if case.kind == "mixed" and case.B >= 3:
        where = torch.randperm(case.B, generator=g)[:2]
        ids[where[0]], ids[where[1]] = case.M * HW, -1
    return ids.to(torch.int64).contiguous()


def upstream(case):
    """d_rays [B,6] fp32."""
    return torch.randn(case.B, 6, generator=torch.Generator().manual_seed(case.seed + 3)).contiguous()


def camera_dirs(dtype, h=H, w=W, f=F):
    """[3, h w] camera-frame directions in ``dtype`` from the fp32 focal length (utils/xyz.rays_single_cam)."""
    f = float(np.float32(f))
    rows = (torch.arange(h) - h // 2).reshape(h, 1).expand(h, w).to(dtype)
    cols = (torch.arange(w) - w // 2).reshape(1, w).expand(h, w).to(dtype)
    return torch.stack((cols / f, -rows / f, -torch.ones_like(cols))).reshape(3, -1)


def valid_rows(ids, M, hw=H * W):
    return (ids >= 0) & (ids < M * hw)


def skew_batch(w):
    """input_grad_model.skew over a leading axis: [M,3] -> [M,3,3]."""
    z = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], 1), torch.stack([w[:, 2], z, -w[:, 0]], 1),
                        torch.stack([-w[:, 1], w[:, 0], z], 1)], 1)


def ray_table(xi, poses0, dirs):
    """input_grad_model.pose_rays of every image, batched: [M hw, 6] in the dtype of xi (test_camera_cpu.py holds it
    against the per-image call)."""
    p = poses0.to(xi.dtype)
    R = torch.linalg.matrix_exp(skew_batch(xi[:, :3])) @ p[:, :, :3]
    d = (R @ dirs).transpose(1, 2)                                                      # [M, hw, 3]
    t = (p[:, :, 3] + xi[:, 3:])[:, None, :].expand_as(d)
    return torch.cat([t, d], dim=2).reshape(-1, 6)


def rays(xi, poses0, ids, dirs):
    """The table's rows by id: [B,6] in the dtype of xi (NaN rows for bad ids)."""
    M, hw = poses0.shape[0], dirs.shape[1]
    table = ray_table(xi, poses0, dirs)
    ok = valid_rows(ids, M, hw)
    out = table[torch.where(ok, ids, torch.zeros_like(ids))]
    return torch.where(ok[:, None], out, torch.full_like(out, float("nan")))


def model(xi, poses0, ids, d_rays, dirs=None):
    """float64: (rays [B,6], g_xi [M,6], units of rays [B,6], units of g_xi [M,6], conditioned units of the directions [B,3])
    as numpy arrays."""
    dirs = camera_dirs(torch.float64) if dirs is None else dirs
    M, hw = poses0.shape[0], dirs.shape[1]
    x = xi.double().clone().requires_grad_(True)
    r = rays(x, poses0, ids, dirs)
    ok = valid_rows(ids, M, hw)
    (r[ok] * d_rays.double()[ok]).sum().backward()
    g = x.grad.detach()
    # units
    with torch.no_grad():
        E = torch.linalg.matrix_exp(skew_batch(x[:, :3]))
        R = E @ poses0.double()[:, :, :3]
        R_abs = E.abs() @ poses0.double()[:, :, :3].abs()
        safe = torch.where(ok, ids, torch.zeros_like(ids))
        img, pix = safe // hw, safe % hw
        d = dirs[:, pix].T                                                              # [B,3]
        u_dir = EPS * torch.einsum("bkj,bj->bk", R[img].abs(), d.abs())
        u_dir_abs = EPS * torch.einsum("bkj,bj->bk", R_abs[img], d.abs())
        u_dir_abs[~ok] = 0.0
        u_org = EPS * (poses0.double()[:, :, 3].abs() + x[:, 3:].abs())[img]
        u_rays = torch.cat([u_org, u_dir], dim=1)
        u_rays[~ok] = 0.0
        y = r[:, 3:].detach()
        per_row_w = torch.where(ok, y.norm(dim=1) * d_rays.double()[:, 3:].norm(dim=1), torch.zeros(len(ids), dtype=torch.float64))
        per_row_t = torch.where(ok[:, None], d_rays.double()[:, :3].abs(), torch.zeros(len(ids), 3, dtype=torch.float64))
        u_g = torch.zeros(M, 6, dtype=torch.float64)
        u_g[:, :3].index_add_(0, img, per_row_w[:, None].expand(-1, 3).contiguous())
        u_g[:, 3:].index_add_(0, img, per_row_t)
        u_g *= EPS
    return r.detach().numpy(), g.numpy(), u_rays.numpy(), u_g.numpy(), u_dir_abs.numpy()


def coefficients(theta):
    """(b, c) of the left Jacobian in float64; their Taylor series where the closed forms cancel."""
    if theta < 1e-2:
        x = theta * theta
        return 0.5 - x / 24 + x * x / 720, 1.0 / 6 - x / 120 + x * x / 5040
    return (1.0 - math.cos(theta)) / theta ** 2, (theta - math.sin(theta)) / theta ** 3


def identity_grad(xi, poses0, ids, d_rays, dirs=None):
    """g_xi [M,6] in float64 by the expression the backward kernel evaluates: g_tau = sum g_o, g_w = J^T sum (y x g_d)."""
    dirs = camera_dirs(torch.float64) if dirs is None else dirs
    M, hw = poses0.shape[0], dirs.shape[1]
    x, g = xi.double(), d_rays.double()
    r = rays(x, poses0, ids, dirs)
    ok = valid_rows(ids, M, hw)
    img = torch.where(ok, ids, torch.zeros_like(ids)) // hw
    s = torch.zeros(M, 3, dtype=torch.float64).index_add_(0, img[ok], torch.linalg.cross(r[ok, 3:], g[ok, 3:]))
    out = torch.zeros(M, 6, dtype=torch.float64)
    out[:, 3:].index_add_(0, img[ok], g[ok, :3])
    for m in range(M):
        K = IG.skew(x[m, :3])
        b, c = coefficients(float(x[m, :3].norm()))
        J = torch.eye(3, dtype=torch.float64) + b * K + c * (K @ K)
        out[m, :3] = J.T @ s[m]
    return out.numpy()


def ratio(got, want, unit):
    """max |got - want| / unit (0 / 0 = 0; a miss where the unit is 0 is +inf; NaN must meet NaN)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    err = np.nan_to_num(np.abs(got - want), nan=0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / unit)
    return float(r.max()) if r.size else 0.0


def case_inputs(case, theta):
    return corrections(case.M, theta, case.seed), stored_poses(case.M, case.seed), ray_ids(case), upstream(case)


def reference_fp32(xi, poses0, ids, d_rays):
    """torch's own fp32 evaluation of the same expression: (rays, g_xi)."""
    dirs = camera_dirs(torch.float32)
    x = xi.clone().requires_grad_(True)
    r = rays(x, poses0, ids, dirs)
    ok = valid_rows(ids, poses0.shape[0])
    (r[ok] * d_rays[ok]).sum().backward()
    return r.detach().numpy(), x.grad.numpy()


def measure(which=None):
    """(c_dir, c_origin, c_gw, c_gtau, c_dir_conditioned): the fp32 reference against the float64 model over cases() x THETAS."""
    c = [0.0, 0.0, 0.0, 0.0, 0.0]
    for case in which or cases():
        for theta in THETAS:
            xi, poses0, ids, g = case_inputs(case, theta)
            r64, g64, u_r, u_g, u_abs = model(xi, poses0, ids, g)
            r32, g32 = reference_fp32(xi, poses0, ids, g)
            c[0] = max(c[0], ratio(r32[:, 3:], r64[:, 3:], u_r[:, 3:]))
            c[1] = max(c[1], ratio(r32[:, :3], r64[:, :3], u_r[:, :3]))
            c[2] = max(c[2], ratio(g32[:, :3], g64[:, :3], u_g[:, :3]))
            c[3] = max(c[3], ratio(g32[:, 3:], g64[:, 3:], u_g[:, 3:]))
            c[4] = max(c[4], ratio(r32[:, 3:], r64[:, 3:], u_abs))
    return tuple(c)


# ---- pose recovery over three images ---------------------------------------------------------------------------------------
REC_HW, REC_N, REC_LR, REC_STEPS, REC_LEVELS = 24, 32, 2e-3, 30, 3
REC_POSES = ((4, -30, 0), (4, -45, 120), (4, -20, 240))           # spherical (r, theta deg, phi deg)


def recovery_start():
    """xi [3,6] fp32: input_grad_model.start_perturbation about a different axis per image (its components permuted)."""
    p = IG.start_perturbation()
    return torch.stack([torch.cat([p[:3][list(o)], p[3:][list(o)]]) for o in ((0, 1, 2), (1, 2, 0), (2, 0, 1))]).contiguous()


def recovery_error(xi):
    return sum(IG.pose_error(xi[m], torch.zeros(6)) for m in range(xi.shape[0]))


def recovery_scene():
    """(smooth state dict, stored poses [3,4,4] fp32, cam_params) of the three-image scene."""
    from nerf_simple_amd.utils import synthetic
    from nerf_simple_amd.utils.xyz import spherical_to_pose
    sd = IG.smooth_state_dict(synthetic.synthetic_state_dict(0, "structured"), REC_LEVELS)
    poses = torch.stack([torch.from_numpy(spherical_to_pose(*p)).float() for p in REC_POSES])
    return sd, poses, [REC_HW, REC_HW, synthetic.focal_from_fov(REC_HW)]


def oracle_recovery(fresh, N):
    """The factor by which 30 Adam steps on the fp32 CPU oracle cut the summed pose error (all 3 x 24 x 24 rays per step)."""
    sd, poses, cam = recovery_scene()
    dirs = camera_dirs(torch.float32, cam[0], cam[1], cam[2])
    ids = torch.arange(3 * REC_HW * REC_HW)
    g = torch.Generator().manual_seed(0)
    u = torch.rand(len(ids), N, generator=g)
    with torch.no_grad():
        target = IG.render(IG.exact_forward, sd, rays(torch.zeros(3, 6), poses[:, :3], ids, dirs), N, u=u)[0]
    xi = recovery_start().clone().requires_grad_(True)
    opt = torch.optim.Adam([xi], lr=REC_LR)
    e0 = recovery_error(xi.detach())
    for _ in range(REC_STEPS):
        if fresh:
            u = torch.rand(len(ids), N, generator=g)
        opt.zero_grad()
        IG.ray_loss(IG.render(IG.exact_forward, sd, rays(xi, poses[:, :3], ids, dirs), N, u=u), target).backward()
        opt.step()
    return e0 / recovery_error(xi.detach())


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "recovery":
        print("RECOVERY_F_FIXED =", oracle_recovery(False, REC_N))
        for N in (32, 64, 128):
            print(f"fresh jitter, N = {N}: F =", oracle_recovery(True, N))
    else:
        print("C_REF_CAM_DIR, C_REF_CAM_ORIGIN, C_REF_CAM_GW, C_REF_CAM_GTAU, C_REF_CAM_DIR_COND =", measure())
