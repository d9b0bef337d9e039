"""Training with the occupancy grid without a GPU: the library's host side (exports, ABI, argument checking of the two new
entry points -- nothing touches a device), the float64 restatement of the masked loss (tests/occupancy_train_model.py)
against central differences, the restated decay-max and its bits, and the inputs of the GPU tests
(tests/test_gpu_occupancy_training.py): every masked input is informative by occupancy_model.require_informative."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import occupancy_model as M
import occupancy_train_model as T

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R129 = (129, 129, 129)
NEW = ("nerf_amd_volume_render_masked_backward", "nerf_amd_occupancy_decay_max")
EINVAL, EUNSUP = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- the library without a GPU -----------------------------------------------------------------------------------------
def test_new_symbols_exported_bound_and_abi_unchanged(lib):
    from nerf_simple_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    for s in NEW:
        assert hasattr(raw, s) and s in _lib.EXPORTS and getattr(lib, s).argtypes is not None, s
        assert re.search(r"\b" + s + r"\(", header), s
    assert lib.nerf_amd_abi_version() == 5


def test_entry_points_refuse_bad_arguments_on_the_host(lib):
    """Every call below must return before anything is launched: the pointers are fake."""
    P = ctypes.c_void_p(0x1000)           # a non-null, 16-aligned address that is never dereferenced
    bw = lib.nerf_amd_volume_render_masked_backward

    def backward(raw=P, rays=P, u=P, tbins=P, flags=0, mask=P, offs=P, g=(P, P, P, P, P), d=P, B=4, N=64):
        return bw(raw, rays, u, tbins, flags, 0, 0, mask, offs, *g, d, B, N, None)
    for kw in (dict(rays=None), dict(u=None), dict(tbins=None), dict(mask=None), dict(offs=None), dict(B=-1), dict(N=0),
               dict(N=-3), dict(flags=16), dict(flags=128), dict(flags=4), dict(raw=None), dict(d=None),
               dict(raw=ctypes.c_void_p(0x1004)), dict(d=ctypes.c_void_p(0x1008)), dict(mask=ctypes.c_void_p(0x1004)),
               dict(offs=ctypes.c_void_p(0x1004))):
        assert backward(**kw) == EINVAL, kw
    assert backward(N=513) == EUNSUP and backward(N=768) == EUNSUP and backward(N=769) == EUNSUP
    assert backward(N=513, g=(None,) * 5) == EUNSUP
    assert backward(B=0) == 0 and backward(B=0, raw=None, d=None) == 0
    dm = lib.nerf_amd_occupancy_decay_max
    assert dm(None, P, 0.95, 8, None) == EINVAL and dm(P, None, 0.95, 8, None) == EINVAL
    assert dm(P, P, 0.95, -1, None) == EINVAL
    for decay in (-0.1, 1.5, float("nan"), float("inf")):
        assert dm(P, P, decay, 8, None) == EINVAL, decay
    assert dm(P, P, 0.95, 0, None) == 0 and dm(None, None, 1.0, 0, None) == 0


def test_python_surface_and_cpu_refusals():
    from nerf_simple_amd import training
    from nerf_simple_amd.utils import nets, occupancy
    assert issubclass(occupancy.TrainingOccupancyGrid, occupancy.OccupancyGrid)
    assert inspect.signature(training.train_step).parameters["occupancy"].default is None
    sig = inspect.signature(training.render_nerf_masked)
    assert list(sig.parameters)[:4] == ["rays", "net", "N", "occupancy"]
    assert inspect.signature(occupancy.TrainingOccupancyGrid.update).parameters["level"].default is inspect.Parameter.empty
    with pytest.raises(RuntimeError, match="GPU"):
        occupancy.TrainingOccupancyGrid(16, device="cpu")
    # CPU rays raise before the grid is looked at, and leave torch's generator alone
    net = nets.Nerf()
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="GPU"):
        training.render_nerf_masked(torch.zeros(2, 6), net, 8, object())
    assert torch.equal(torch.get_rng_state(), state)
    # the host-side threshold is the model's
    for level in (-30.0, -1.75, 0.0, 3.0, 19.99, 20.0, 20.5, 100.0):
        assert np.float32(occupancy.softplus_level(level)) == T.softplus32(level), level


# ---- the masked loss: autograd against central differences -------------------------------------------------------------
def step_inputs(oracle, synthetic, B, N):
    """the rays, targets and jitter of tests/test_gpu_training.py::test_fused_training_vs_oracle at this shape"""
    gen = torch.Generator().manual_seed(B * 1000 + N)
    pose = torch.from_numpy(oracle.spherical_to_pose(4, -30, 0)).float()
    side = int(np.ceil(np.sqrt(B)))
    rays = oracle.camera_rays(pose, [side, side, synthetic.focal_from_fov(side)])[:B].contiguous()
    gt = torch.rand(B, 3, generator=gen)
    u = torch.rand(B, N, generator=gen)
    return rays, gt, u


@pytest.mark.parametrize("outside", ["empty", "live"])
def test_masked_loss_autograd_agrees_with_central_differences(oracle, synthetic, outside):
    B, N = 37, 65
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    ts, q, dn = T.geometry(rays, u=u)
    live = T.live_of(q, M.ball_cells(R129, BOUNDS, 1.0), R129, BOUNDS, outside)
    M.require_informative(live, N, outside)
    gen = torch.Generator().manual_seed(5)
    raw_live = torch.randn(int(live.sum()), 4, generator=gen, dtype=torch.float64)
    raw_live[:, 3] = raw_live[:, 3] * 2 - 1
    coef = [torch.randn(s, generator=gen, dtype=torch.float64) for s in ((B, 3), (B,), (B, N), (B,), (B, N))]
    has = torch.from_numpy(live.sum(1) > 0)

    def f(x):
        rgb, disp, alpha, acc, w = T.masked_outputs(x, ts.double(), dn.double(), live)
        # a ray with no live sample has NaN disparity (acc = 0), which depends on nothing: left out of the sum
        return (torch.nn.functional.mse_loss(rgb, gt.double()) + (coef[0] * rgb).sum() + (coef[1] * disp)[has].sum()
                + (coef[2] * alpha).sum() + (coef[3] * acc).sum() + (coef[4] * w).sum())

    x = raw_live.clone().requires_grad_(True)
    f(x).backward()
    assert torch.isfinite(x.grad).all()
    rng = np.random.default_rng(0)
    idx = rng.choice(raw_live.numel(), 40, replace=False)
    with torch.no_grad():
        cd = T.central_differences(f, raw_live, idx, 1e-6)
    ag = x.grad.reshape(-1)[idx].numpy()
    assert np.abs(cd - ag).max() <= 1e-6 * max(1.0, np.abs(ag).max()), np.abs(cd - ag).max()
    # the dense gradient at the dead rows is exactly zero: a dead sample receives nothing
    dense = T.scatter_live(raw_live, live).requires_grad_(True)
    outs = oracle.volume_render(dense, ts.double(), dn.double())
    (outs[0].sum() + outs[3].sum() + (coef[4] * outs[4]).sum() + (coef[2] * outs[2]).sum()).backward()
    assert (dense.grad[torch.from_numpy(~live)] == 0).all()


def test_masked_loss_of_an_empty_batch_is_mean_gt_squared(oracle, synthetic):
    B, N = 16, 8
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    ts, q, dn = T.geometry(rays, u=u)
    live = np.zeros((B, N), bool)
    sd = synthetic.synthetic_state_dict(0, "default")
    import input_grad_model as IG

    def loss_of(forward, sdp, dtype):
        return T.masked_loss(forward, sdp, q, ts, dn, live, gt, dtype)
    loss, grads = T.param_grads(loss_of, IG.exact_forward, sd, torch.float64)
    assert abs(loss - float((gt.double() ** 2).mean())) <= 1e-15
    assert all((g == 0).all() for g in grads.values())


# ---- the inputs of the GPU tests are informative -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(576, 64), (37, 65)])
def test_step_level_inputs_are_informative(oracle, synthetic, shape):
    B, N = shape
    rays, _, u = step_inputs(oracle, synthetic, B, N)
    _, q, _ = T.geometry(rays, u=u)
    for outside in ("empty", "live"):
        live = T.live_of(q, M.ball_cells(R129, BOUNDS, 1.0), R129, BOUNDS, outside)
        frac, _, _ = M.require_informative(live, N, outside)
        assert 0.05 <= frac <= 0.95


@pytest.mark.parametrize("N", [1, 3, 64, 65, 128, 512])
def test_kernel_level_inputs_are_informative(oracle, synthetic, N):
    """the 100 x 100 view of tests/test_gpu_occupancy.py at the kernel-level test's sample counts"""
    pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, 30, 45))).float()
    rays = oracle.camera_rays(pose, [100, 100, synthetic.focal_from_fov(100)])
    torch.manual_seed(0)
    _, q, _ = T.geometry(rays, u=torch.rand(10000, N))
    for outside in ("empty", "live"):
        M.require_informative(T.live_of(q, M.ball_cells(R129, BOUNDS, 1.0), R129, BOUNDS, outside), N, outside)


def scene_views(oracle, synthetic, side=32):
    """the end-to-end test's cameras: training views on the radius-4 sphere and one held-out view"""
    cam = [side, side, synthetic.focal_from_fov(side)]
    train = [(30, 0), (30, 90), (30, 180), (30, 270), (-20, 45), (-20, 225), (60, 135)]
    rays = [oracle.camera_rays(torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, th, ph))).float(), cam) for th, ph in train]
    held = oracle.camera_rays(torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, 10, 300))).float(), cam)
    return torch.cat(rays).contiguous(), held.contiguous()


def test_end_to_end_scene_is_mostly_empty(oracle, synthetic):
    """The analytic ball (radius 0.75) under a 128^3 grid over [-1, 1]^3, outside = 'empty': even the ball's cells dilated
    by the grid's own corner rule and one cell keep far fewer than half of the samples of the training rays alive."""
    R, bounds = (128, 128, 128), ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    rays, held = scene_views(oracle, synthetic)
    torch.manual_seed(1)
    _, q, _ = T.geometry(rays, u=torch.rand(rays.shape[0], 64))
    lo, step, _ = M.grid_axes(R, bounds)
    ax = [lo[a] + np.arange(R[a], dtype=np.float32) * step[a] for a in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    sigma = np.where(X * X + Y * Y + Z * Z <= T.BALL_RADIUS ** 2, T.SIGMA_IN, T.SIGMA_OUT).astype(np.float32)
    cells = T.cells_from_state(T.softplus32(sigma), -1.75, 1)
    live = T.live_of(q, cells, R, bounds, "empty")
    frac = float(live.mean())
    assert 0.02 < frac < 0.15, frac
    # the targets see the ball: a good share of the pixels is covered, and the rest is black (to 1e-5)
    tgt = T.scene_targets(held)
    assert float((tgt.sum(1) > 0.1).float().mean()) > 0.1 and float((tgt.sum(1) < 1e-5).float().mean()) > 0.3


# ---- the running density volume ------------------------------------------------------------------------------------------------
def test_decay_max_model_and_its_bits():
    rng = np.random.default_rng(3)
    R = (9, 7, 38)
    state = np.abs(rng.normal(size=R)).astype(np.float32) * 4
    sigma = (rng.normal(size=R) * 8).astype(np.float32)
    out = T.decay_max(state, sigma, 0.95)
    assert out.dtype == np.float32 and (out >= 0).all()
    assert (out >= T.softplus32(sigma)).all() and (out >= (state * np.float32(0.95)).astype(np.float32)).all()
    # identity above 20: exact, and the decay product is one float32 multiply
    big = (rng.random(R) * 50 + 20.5).astype(np.float32)
    assert np.array_equal(T.decay_max(state, big, 0.95), np.maximum((state * np.float32(0.95)).astype(np.float32), big))
    # inexact part: numpy-fp32 sits inside its own bound of the float64 value
    want, scale, bound = T.decay_max_bound(state, sigma, 0.95)
    assert np.abs(out - want).max() / scale <= bound
    # NaN propagates from either side, and is live in the bits
    s2, g2 = state.copy(), sigma.copy()
    s2[1, 1, 1], g2[2, 2, 2] = np.nan, np.nan
    o2 = T.decay_max(s2, g2, 0.95)
    assert np.isnan(o2[1, 1, 1]) and np.isnan(o2[2, 2, 2]) and np.isnan(o2).sum() == 2
    cells = T.cells_from_state(np.where(np.isnan(o2), np.nan, 0).astype(np.float32), 0.0, 0)
    assert cells[:2, :2, :2].all() and cells[1:3, 1:3, 1:3].all() and cells.sum() == 15
    # bits: the state against softplus(level) with the corner rule
    for level, dilate in ((-1.75, 1), (2.0, 0), (25.0, 2)):
        c = T.cells_from_state(out, level, dilate)
        assert np.array_equal(c, M.cells_from_density(out, float(T.softplus32(level)), dilate))
        assert np.array_equal(c, M.cells_from_density_direct(out, float(T.softplus32(level)), dilate))
    # a zero state (a fresh grid) with any level is dead everywhere once updated from nothing; softplus > 0 keeps it >= 0
    assert not T.cells_from_state(np.zeros(R, np.float32), -1.75, 1).any()


def test_steps_until_dead():
    # softplus(8) decayed by 0.95 against softplus(-1.75) = 0.1602...: 0.95^k * 8.000335 <= 0.1602 first at k = 77
    k = T.steps_until_dead(T.softplus32(8.0), 0.95, -1.75)
    exact = int(np.ceil(np.log(float(T.softplus32(-1.75)) / float(T.softplus32(8.0))) / np.log(0.95)))
    assert abs(k - exact) <= 1 and k == 77
    assert T.steps_until_dead(1.0, 0.5, float(np.log(np.expm1(0.26)))) == 2
    assert T.steps_until_dead(1.0, 0.0, -1.75) == 1


def test_new_kernels_pass_the_static_isa_checks():
    """tools/check_vmcnt.py on csrc/occupancy_train.hip (tests/static_isa.py): no counted vmcnt wait is short, no wide store
    has its data registers overwritten by the next instruction, no atomic.  The source holds the six plain instantiations of
    the masked compositor backward -- the eager backward's is (FiveGrads, 0) --, the seven of the head with a training control
    on (noise, background, distortion; no sampler), the twelve of the pair's coarse head with a control on (noise, background;
    the sampler at E = 1, 2, 4, 8), and occ_decay_max_kernel, and nothing else."""
    import static_isa
    kernels = static_isa.checked_kernels("occupancy_train.hip")
    assert static_isa.masked_backward_instantiations(kernels) == \
        [("FiveGrads", 0), ("MseHead", 0), ("MseHead", 1), ("MseHead", 2), ("MseHead", 4), ("MseHead", 8)], list(kernels)
    assert static_isa.masked_term_instantiations(kernels) == \
        sorted([(n, b, d, 0) for n in (0, 1) for b in (0, 1) for d in (0, 1) if n or b or d] +
               [(n, b, 0, e) for n, b in ((0, 1), (1, 0), (1, 1)) for e in (1, 2, 4, 8)]), list(kernels)
    assert len(kernels) == 26 and sum("occ_decay_max_kernel" in k for k in kernels) == 1, list(kernels)
