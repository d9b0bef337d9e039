"""numpy / torch restatement of early ray termination (include/nerf_amd.h, "terminated render"; csrc/occupancy_terminate.hip;
DESIGN.md section 16).  Test infrastructure.

A ray's N samples are cut into slabs of S sample indices; before slab k the transmittance T_k over the rows evaluated so far is
formed (T_0 = 1); the ray is terminated from slab k on iff T_k < eps (a NaN T_k is not terminated); a terminated ray evaluates
nothing more and its T is frozen.  M* = M0 & (the slab of sample i is not terminated), and the terminated render is the
masked render (tests/occupancy_model.py) under M*."""
import numpy as np
import torch

import occupancy_model as M

F32 = np.float32
SLABS = (16, 32, 64)


def slab_count(N, S):
    return -(-N // S)


def slab_bounds(N, S):
    """[(s0, s1)] of the K slabs; the last one may be short"""
    return [(k * S, min(k * S + S, N)) for k in range(slab_count(N, S))]


def advance_calls(N, S):
    """(s0, s1, s2) of the K + 1 calls of nerf_amd_termination_advance: select slab 0, then retire slab k and select slab k + 1"""
    b = slab_bounds(N, S)
    calls = [(0, 0, b[0][1])]
    for k, (s0, s1) in enumerate(b):
        calls.append((s0, s1, b[k + 1][1] if k + 1 < len(b) else N))
    return calls


def alphas(raw, ts, dirs):
    """alpha [B, N] of raw [B, N, 4] by the oracle's formulas (reference utils/rendering.py:60-66), in raw's dtype"""
    deltas = torch.cat((ts[:, 1:] - ts[:, :-1], 1e10 * torch.ones_like(ts[:, :1])), dim=1)
    deltas = deltas * torch.norm(dirs[..., None, :], dim=-1)
    return 1 - torch.exp(-torch.nn.functional.softplus(raw[..., 3]) * deltas)


def factor32(alpha):
    """the compositor's factor fl(fl(1 - alpha) + 1e-10) in float32; never above 1"""
    a = np.asarray(alpha, dtype=F32)
    with np.errstate(invalid="ignore"):
        return ((F32(1) - a).astype(F32) + F32(1e-10)).astype(F32)


def terminate(alpha, live0, S, eps, dtype=np.float64, exact_factor=False):
    """The evaluation rule on alpha [B, N] (of every sample, were it evaluated) and the occupancy mask live0 [B, N].
    Returns (T [B, K] in `dtype`, evaluated bool [B, N] = M*, terminated bool [B, K]).  The factors are the compositor's float32
    ones (exact_factor: 1 - alpha + 1e-10 formed in `dtype`), their running product is kept in `dtype`, sample order."""
    alpha = np.asarray(alpha)
    live0 = np.asarray(live0, dtype=bool)
    B, N = alpha.shape
    K = slab_count(N, S)
    fac = (1 - alpha.astype(dtype) + dtype(1e-10)) if exact_factor else factor32(alpha).astype(dtype)
    T = np.ones(B, dtype=dtype)
    Tk = np.ones((B, K), dtype=dtype)
    evaluated = np.zeros((B, N), dtype=bool)
    terminated = np.zeros((B, K), dtype=bool)
    eps = dtype(eps)
    for k, (s0, s1) in enumerate(slab_bounds(N, S)):
        Tk[:, k] = T
        with np.errstate(invalid="ignore"):
            terminated[:, k] = T < eps                               # NaN: not terminated
        alive = ~terminated[:, k]
        evaluated[:, s0:s1] = live0[:, s0:s1] & alive[:, None]
        nxt = T.copy()
        for i in range(s0, s1):
            nxt = np.where(evaluated[:, i], nxt * fac[:, i], nxt)
        T = np.where(alive, nxt, T)                                  # a terminated ray's T is frozen
    return Tk, evaluated, terminated


def terminated_composite(raw, ts, dirs, live0, S, eps):
    """A composite that stops: the walk of occupancy_model.live_only_composite (weights from the oracle's formulas, the ray sums
    accumulated in sample order over the evaluated samples alone), with the slab rule applied to its own running transmittance.
    Returns ((rgb, depth, acc, alpha, w), T [B, K], evaluated bool [B, N])."""
    live0 = torch.from_numpy(np.asarray(live0, dtype=bool))
    B, N = ts.shape
    K = slab_count(N, S)
    a_all = alphas(raw, ts, dirs)
    alpha = torch.zeros_like(ts)
    w = torch.zeros_like(ts)
    T = torch.ones(B, dtype=torch.float64)      # torch.cumprod on the CPU accumulates float32 factors in double
    rgb = torch.zeros(B, 3, dtype=ts.dtype)
    depth = torch.zeros(B, dtype=ts.dtype)
    acc = torch.zeros(B, dtype=ts.dtype)
    alive = torch.ones(B, dtype=torch.bool)
    Tk = torch.ones(B, K, dtype=ts.dtype)
    evaluated = torch.zeros(B, N, dtype=torch.bool)
    for i in range(N):
        if i % S == 0:
            Tk[:, i // S] = torch.where(alive, T.to(ts.dtype), Tk[:, max(i // S - 1, 0)])
            alive = alive & ~(Tk[:, i // S] < eps)
        m = live0[:, i] & alive
        evaluated[:, i] = m
        a = a_all[:, i]
        wi = a * T.to(ts.dtype)
        alpha[:, i] = torch.where(m, a, alpha[:, i])
        w[:, i] = torch.where(m, wi, w[:, i])
        rgb = torch.where(m[:, None], rgb + wi[:, None] * raw[:, i, :3], rgb)
        depth = torch.where(m, depth + wi * ts[:, i], depth)
        acc = torch.where(m, acc + wi, acc)
        # an unevaluated sample's factor is 1 - 0 + 1e-10 as the dtype rounds it: exactly 1 in float32 (occupancy_model.py)
        T = T * torch.where(m, 1. - a + 1e-10, 1. - torch.zeros_like(a) + 1e-10).double()
    return (rgb, depth, acc, alpha, w), Tk, evaluated.numpy()


def bounds(raw, evaluated, live0, eps):
    """per ray: (eps max|c| over the dropped samples [B], eps) -- what rgb / acc may move by against the un-terminated masked
    render (the dropped samples' weights sum to less than the transmittance that reached them, < eps)"""
    dropped = torch.from_numpy(np.asarray(live0, dtype=bool) & ~np.asarray(evaluated, dtype=bool))
    c = raw[..., :3].abs().amax(-1)
    cmax = torch.where(dropped, c, torch.zeros_like(c)).amax(1)
    return eps * cmax, eps


def terminated_share(terminated):
    """share of the rays that are terminated at the last check, i.e. skip at least their last slab"""
    return float(np.asarray(terminated)[:, -1].mean())


def masked_composite(oracle, raw, ts, dirs, evaluated):
    return M.masked_composite(oracle, raw, ts, dirs, evaluated)


BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R129 = (129, 129, 129)
_cache = {}


def view(oracle, synthetic, N, n_side=20):
    """The inputs the termination tests share: camera spherical_to_pose(4, -30, 40), n_side x n_side rays, t in [2, 6],
    torch.manual_seed(0) jitter.  Returns (pose, rays [B, 6], u [B, N], ts [B, N], q [B, N, 6], dirs [B, 3])."""
    key = ("view", N, n_side)
    if key not in _cache:
        pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, -30, 40))).float()
        rays = oracle.camera_rays(pose, [n_side, n_side, synthetic.focal_from_fov(n_side)]).contiguous()
        state = torch.get_rng_state()
        torch.manual_seed(0)
        u = torch.rand(rays.shape[0], N)
        torch.set_rng_state(state)
        ts = oracle.sample_ts(u)
        q, dn = oracle.query_points(rays, ts)
        _cache[key] = (pose, rays, u, ts, q.reshape(rays.shape[0], N, 6), dn)
    return _cache[key]


def view_raw(oracle, synthetic, kind, N, n_side=20, sigma_shift=0.0):
    """the oracle's network output [B, N, 4] on those points, for the synthetic weight set `kind`"""
    key = ("raw", kind, N, n_side, sigma_shift)
    if key not in _cache:
        sd = synthetic.synthetic_state_dict(0, kind)
        if sigma_shift:
            sd = {k: v.clone() for k, v in sd.items()}
            sd["sigma_fc.0.bias"] += sigma_shift
        q = view(oracle, synthetic, N, n_side)[4]
        with torch.no_grad():
            _cache[key] = oracle.nerf_forward(sd, q.reshape(-1, 6)).reshape(q.shape[0], N, 4)
    return _cache[key]


def view_live(oracle, synthetic, grid, N, n_side=20):
    """M0 of those points: grid 'all' (every sample) or 'ball' (the radius-1 ball in a 129^3 grid, outside = empty)"""
    q = view(oracle, synthetic, N, n_side)[4]
    if grid == "all":
        return np.ones(q.shape[:2], dtype=bool)
    key = ("live", N, n_side)
    if key not in _cache:
        lo, _, inv = M.grid_axes(R129, BOUNDS)
        if "ball" not in _cache:
            _cache["ball"] = M.ball_cells(R129, BOUNDS, 1.0)
        _cache[key] = M.sample_live(q[..., :3].numpy(), _cache["ball"], lo, inv, "empty")
    return _cache[key]
