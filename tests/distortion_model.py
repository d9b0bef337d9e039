"""Float64 model of the distortion loss (test infrastructure; uses the oracle's compositor for the weights and
tests/ray_routines_model.py / tests/background_model.py for the head, and edits none of them).

Definition (include/nerf_amd.h, restated): for one ray with positions t_0 <= ... <= t_{N-1}, weights w and the far plane t_far
    delta_i = t_{i+1} - t_i (i < N - 1),  delta_{N-1} = max(t_far - t_{N-1}, 0),  m_i = t_i + delta_i / 2
    D       = 2 sum_i w_i sum_{j<i} w_j (m_i - m_j) + (1/3) sum_i w_i^2 delta_i
    dD/dw_i = 2 [ sum_{j<i} w_j (m_i - m_j) + sum_{j>i} w_j (m_j - m_i) ] + (2/3) w_i delta_i
N == 1 is the reference's empty sample axis: D = 0 and no gradient.

Units (functions of the float64 intermediates only; EPS = 2^-24):
    gradient to w_i:   unit_i = EPS [ sum_j |w_j| (|m_i| + |m_j|) + |w_i| delta_i ]
    D:                 unit   = EPS [ sum_ij |w_i| |w_j| (|m_i| + |m_j|) + sum_i w_i^2 delta_i ]
each scaled by the launch's coef.  They are what one rounding of every product w_j m_j and w_j m_i costs: the sums the O(N)
algorithm and the direct O(N^2) expression both form.  A value whose unit is 0 (all-zero weights) must be met exactly.

Constants.  C_REF_DIST_GW / C_REF_DIST_LOSS: the largest ratio of torch's direct O(N^2) fp32 expression
sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i (and its fp32 autograd) against float64 over cases().  The head:
C_REF_DIST_HEAD / C_REF_DIST_HEAD_PLAIN, the two per-ray ratios of ray_routines_model.ray_ratios for the reference's own fp32
evaluation of the TOTAL loss MSE(rgb + (1 - acc) bg, gt) + coef sum_rays D (oracle.volume_render + blend + MSE + the direct
expression, fp32 autograd) against the float64 model, whose upstream gradients g_rgb, g_acc, g_w are formed from the float64
forward (as background_model.C_REF_BG was measured).  Written by

    python tests/distortion_model.py            (well under a minute on a CPU; prints the four constants)

rounded up to two digits; tests/test_distortion_cpu.py asserts that the fp32 reference stays inside them and reaches half of
them, and the GPU tests allow ray_routines_model.bound(c) = 2 c + 4.  Nothing here is taken from what a GPU shows.
"""
import os
import sys
from collections import namedtuple

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "oracle"), os.path.join(_ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import nerf_oracle as O  # noqa: E402
import ray_routines_model as M  # noqa: E402
import background_model as BM  # noqa: E402

EPS = M.EPS
TN, TF = 2.0, 6.0

# measured on the CPU by `python tests/distortion_model.py` (see the module docstring)
C_REF_DIST_GW = 3.4
C_REF_DIST_LOSS = 0.67
C_REF_DIST_HEAD = 2.7
C_REF_DIST_HEAD_PLAIN = 11.0

# ---- cases of the stage --------------------------------------------------------------------------------------------------
DistCase = namedtuple("DistCase", "id N B positions weights seed")
DIST_N = (2, 3, 63, 64, 65, 128, 129, 512)
DIST_B = (1, 5, 37)
POSITIONS = ("stratified", "merged")
WEIGHTS = ("rendered", "onehot", "zero", "far")


def cases():
    out = []
    for N in DIST_N:
        for B in DIST_B:
            for p in POSITIONS:
                for wk in WEIGHTS:
                    out.append(DistCase(f"N{N}-B{B}-{p}-{wk}", N, B, p, wk, 7000 + len(out)))
    return out


def _clustered(B, Nc, g):
    """Coarse weights gathered around one bin per ray: what a proposal or a coarse pass hands the sampler near a surface."""
    centre = torch.randint(0, Nc, (B, 1), generator=g).float()
    return torch.exp(-0.5 * ((torch.arange(Nc).float()[None, :] - centre) / 0.7) ** 2)


def positions(case):
    """ts [B,N] fp32, nondecreasing.  'stratified': the reference's bins with seeded jitter.  'merged': oracle.sample_pdf on
    clustered coarse weights, half of its uniforms on a grid of 1/8 -- duplicates and very uneven intervals (at N < 4, below
    the sampler's sizes: stratified positions with a coincident pair)."""
    g = torch.Generator().manual_seed(case.seed)
    B, N = case.B, case.N
    if case.positions == "stratified" or N < 4:
        ts = O.sample_ts(torch.rand(B, N, generator=g), TN, TF)
        if case.positions == "merged":
            ts[:, 1] = ts[:, 0]
        return ts.contiguous()
    Nc = max(3, N // 3)
    Nf = N - Nc
    ts_c = O.sample_ts(torch.rand(B, Nc, generator=g), TN, TF)
    u = torch.rand(B, Nf, generator=g)
    u = torch.where(torch.rand(B, Nf, generator=g) < 0.5, torch.floor(u * 8) / 8, u)
    return O.sample_pdf(ts_c, _clustered(B, Nc, g), u).contiguous()


def inputs(case):
    """(ts [B,N], w [B,N], t_far) in fp32.  'rendered': the oracle's compositor on seeded raw (sigma = 3 N(0,1) - 1 so that the
    weights are spread); 'onehot': one sample per ray; 'zero'; 'far': rendered, the far plane in front of the last samples."""
    ts = positions(case)
    g = torch.Generator().manual_seed(case.seed + 13)
    B, N = case.B, case.N
    t_far = TF
    if case.weights in ("rendered", "far"):
        raw = torch.randn(B, N, 4, generator=g)
        raw[..., 3] = 3.0 * raw[..., 3] - 1.0
        d = torch.randn(B, 3, generator=g)
        w = O.volume_render(raw, ts, d / torch.norm(d, dim=1, keepdim=True))[4]
        if case.weights == "far":
            t_far = float(ts[:, -1].min()) - 0.25 if N > 1 else TF        # t_{N-1} > t_far on every ray
    elif case.weights == "onehot":
        w = torch.zeros(B, N)
        w[torch.arange(B), torch.randint(0, N, (B,), generator=g)] = 1.0
    else:
        w = torch.zeros(B, N)
    return ts, w.contiguous(), t_far


# ---- the float64 model ---------------------------------------------------------------------------------------------------
def intervals(ts, t_far):
    """(delta, m) [B,N] in the dtype of ts."""
    last = torch.clamp(t_far - ts[:, -1:], min=0)
    delta = torch.cat([ts[:, 1:] - ts[:, :-1], last], dim=1)
    return delta, ts + delta / 2


def model(ts, w, t_far, coef=1.0):
    """float64 (D [B], dD/dw [B,N], unit_D [B], unit_g [B,N]) of the ORDERED form, each times coef; numpy."""
    t, w = ts.double(), w.double()
    B, N = t.shape
    if N == 1:
        z = np.zeros
        return z(B), z((B, w.shape[1])), z(B), z((B, w.shape[1]))
    delta, m = intervals(t, float(t_far))
    diff = m[:, :, None] - m[:, None, :]                                  # [b, i, j] = m_i - m_j
    below = torch.tril(torch.ones(N, N, dtype=torch.float64), diagonal=-1)        # j < i
    sgn = below - below.T                                                 # +1 at j < i, -1 at j > i
    D = 2 * (w[:, :, None] * w[:, None, :] * diff * below).sum(dim=(1, 2)) + (w * w * delta).sum(dim=1) / 3
    g = 2 * (w[:, None, :] * diff * sgn).sum(dim=2) + 2 * w * delta / 3
    am = m.abs()[:, :, None] + m.abs()[:, None, :]
    unit_g = EPS * ((w.abs()[:, None, :] * am).sum(dim=2) + w.abs() * delta)
    unit_D = EPS * ((w.abs()[:, :, None] * w.abs()[:, None, :] * am).sum(dim=(1, 2)) + (w * w * delta).sum(dim=1))
    return tuple((coef * x).numpy() for x in (D, g, unit_D, unit_g))


def direct(ts, w, t_far):
    """mip-NeRF 360's |.| form, the direct O(N^2) expression, in the dtype of the inputs: D [B] (differentiable in w)."""
    delta, m = intervals(ts, t_far)
    return (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum(dim=(1, 2)) + (w * w * delta).sum(dim=1) / 3


def prefix_form(ts, w, t_far):
    """The kernel's algebra in float64: (D [B], dD/dw [B,N]) from the four running sums, midpoints centred on t_0."""
    t, w = ts.double(), w.double()
    delta, m = intervals(t, float(t_far))
    m = m - t[:, :1]
    wm = w * m
    P, Q = torch.cumsum(w, 1) - w, torch.cumsum(wm, 1) - wm
    S, R = w.sum(1, keepdim=True) - torch.cumsum(w, 1), wm.sum(1, keepdim=True) - torch.cumsum(wm, 1)
    a = m * P - Q
    return (w * 2 * a).sum(1) + (w * w * delta).sum(1) / 3, 2 * (a + (R - m * S)) + 2 * w * delta / 3


def ratio(got, want, unit):
    """max |got - want| / unit (0 / 0 = 0; a miss where the unit is 0 is +inf)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / unit)
    return float(r.max()) if r.size else 0.0


def direct_fp32(ts, w, t_far):
    """(D [B], dD/dw [B,N]) of torch's direct expression and its autograd in fp32, as float64 numpy."""
    wl = w.clone().requires_grad_(True)
    D = direct(ts, wl, t_far)
    D.sum().backward()
    return D.detach().double().numpy(), wl.grad.double().numpy()


# ---- the head ------------------------------------------------------------------------------------------------------------
HEAD_LAMBDA = 1.0
HEAD_MODES = ("neither", "bgB")


def head_cases():
    """background_model's head cases, the background alternating: (case, mode)."""
    return [(c, HEAD_MODES[k % 2]) for k, c in enumerate(BM.head_cases())]


def head_coef(B, lam=HEAD_LAMBDA):
    return lam / (B * (TF - TN))


def head_model(raw, ts, rays, target, bg, coef, t_far=TF):
    """float64 (want [B,N,4], A [B,N,4], rgb_bg [B,3], loss_ray [B], its tolerance [B]) of d (MSE(rgb + (1 - acc) bg, target) +
    coef sum_rays D) / d raw: the compositor's backward with g_rgb, g_acc and g_w = coef dD/dw, all from the float64 forward."""
    dn = BM.unit_dirs(rays)
    fw = M.forward64(raw, ts, dn)
    B = ts.shape[0]
    w = fw["w"]
    rgb = (w[..., None] * raw[..., :3].double()).sum(dim=1)
    acc = w.sum(dim=1)
    b = torch.zeros(B, 3, dtype=torch.float64) if bg is None else bg.double().expand(B, 3)
    rgb_bg = rgb + (1 - acc)[:, None] * b
    g_rgb = 2.0 * (rgb_bg - target.double()) / (3.0 * B)
    g_acc = None if bg is None else -(g_rgb * b).sum(dim=1)
    D, g_w, unit_D, _ = model(ts, w, t_far, coef)
    want, A = M.model_backward(fw, raw, ts, [g_rgb, None, None, g_acc, torch.from_numpy(g_w)])
    # the head's loss values are formed from ITS fp32 weights: beside the stage's own allowance on given weights, the first-order
    # effect of each weight's rounding, EPS T_i (1 + alpha_i kappa_i) (ray_routines_model.model_backward), with the fp32 rule's
    # factor 2
    kappa = 1 + torch.cumsum(1 / fw["f"], dim=1) - 1 / fw["f"]
    dw = EPS * fw["T"] * (1 + fw["alpha"] * kappa)
    tol_D = M.bound(C_REF_DIST_LOSS) * unit_D + 2.0 * (np.abs(g_w) * dw.numpy()).sum(axis=1)
    return want, A, rgb_bg.numpy(), D, tol_D


def total_loss(raw, ts, rays, target, bg, coef, t_far=TF):
    """The total loss through the oracle's compositor in the dtype of ``raw`` (differentiable in raw)."""
    dt = raw.dtype
    rgb, _, _, acc, w = O.volume_render(raw, ts.to(dt), BM.unit_dirs(rays).to(dt))
    if bg is not None:
        rgb = rgb + (1 - acc)[:, None] * bg.to(dt)
    return torch.mean((rgb - target.to(dt)) ** 2) + coef * direct(ts.to(dt), w, t_far).sum()


def oracle_total_grad(raw, ts, rays, target, bg, coef, dtype, t_far=TF):
    r = raw.to(dtype).clone().requires_grad_(True)
    total_loss(r, ts, rays, target, bg, coef, t_far).backward()
    return r.grad.double().numpy()


def measure():
    c_gw = c_loss = 0.0
    for case in cases():
        ts, w, t_far = inputs(case)
        D, g, unit_D, unit_g = model(ts, w, t_far)
        D32, g32 = direct_fp32(ts, w, t_far)
        c_loss, c_gw = max(c_loss, ratio(D32, D, unit_D)), max(c_gw, ratio(g32, g, unit_g))
    return c_gw, c_loss


def measure_head():
    c_cond = c_plain = 0.0
    for case, mode in head_cases():
        raw, ts, rays, target, bg1, bgB = BM.head_inputs(case)
        bg = BM.mode_controls(mode, bg1, bgB)[0]
        coef = head_coef(case.B)
        want, A, _, _, _ = head_model(raw, ts, rays, target, bg, coef)
        ref32 = oracle_total_grad(raw, ts, rays, target, bg, coef, torch.float32)
        cond, plain = M.ray_ratios(ref32, want, A, np.isfinite(ref32))
        c_cond, c_plain = max(c_cond, float(cond.max())), max(c_plain, float(np.nanmax(plain, initial=0.0)))
    return c_cond, c_plain


if __name__ == "__main__":
    print("C_REF_DIST_GW = %.3g   C_REF_DIST_LOSS = %.3g" % measure())
    print("C_REF_DIST_HEAD = %.3g   C_REF_DIST_HEAD_PLAIN = %.3g" % measure_head())
