"""Training with the occupancy grid on the GPU (csrc/occupancy_train.hip, utils/occupancy.TrainingOccupancyGrid,
training.render_nerf_masked / train_step(..., occupancy=)).  Yardsticks: tests/occupancy_train_model.py.

Kernel level: d_raw_live against the rows at the live samples of the dense backward on the overwritten raw, bit for bit
(both kernels run csrc/composite_backward_device.h); decay-max against numpy.
Step level: the all-live grid against the dense points-mode composition; ball grids against the float64 masked model under
the project's model rule; the empty batch; the refusals.  End to end: an analytic ball trained dense and through a
TrainingOccupancyGrid.

Kernel-level inputs: the 100 x 100 view of tests/test_gpu_occupancy.py and its radius-1 ball grid.  Step-level inputs: the
rays of tests/test_gpu_training.py::test_fused_training_vs_oracle.  tests/test_occupancy_training_cpu.py checks on the CPU
model that every one of them is informative.
"""
import json
import os
import time
import warnings

import numpy as np
import pytest
import torch

import occupancy_model as M
import occupancy_train_model as T

pytestmark = pytest.mark.gpu

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R129 = (129, 129, 129)
BS = (1, 63, 1000)
NS = (1, 3, 64, 65, 128, 512)
POLICIES = ("empty", "live")
LOSS_RTOL = {"default": 1e-3, "structured": 2e-2}      # tests/test_gpu_training.py: fp32 compositor on bf16 MLP outputs
SENTINEL = 1234.5
_scene = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def make_net(dev, kind, precision="bf16", sd=None):
    from nerf_simple_amd.utils import synthetic
    from nerf_simple_amd.utils.nets import Nerf
    net = Nerf(precision=precision).to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, kind) if sd is None else sd)
    return net


def full_rays(oracle, synthetic):
    if "rays" not in _scene:
        pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, 30, 45))).float()
        _scene["rays"] = oracle.camera_rays(pose, [100, 100, synthetic.focal_from_fov(100)]).contiguous()
    return _scene["rays"]


def full_u(N):
    if ("u", N) not in _scene:
        torch.manual_seed(0)
        _scene[("u", N)] = torch.rand(10000, N)
    return _scene[("u", N)]


def subset(B):
    return np.array([5050]) if B == 1 else np.linspace(0, 9999, B).astype(np.int64)


def ball_grid(dev, outside):
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    key = ("grid", outside)
    if key not in _scene:
        _scene[key] = OccupancyGrid.from_mask(torch.from_numpy(M.ball_cells(R129, BOUNDS, 1.0)).to(dev), BOUNDS, outside=outside)
    return _scene[key]


def tbins(N, dev):
    from nerf_simple_amd.utils.rendering import _tbins
    return _tbins(2, 6, N, dev)


def query_points(rays, jit, tb, flags, seed, ray_id0, N):
    from nerf_simple_amd.utils.rendering import _query_points
    return _query_points(rays, jit, tb, flags, seed, ray_id0, N)


def unpack_mask(mask, N):
    """MarkResult.mask [B, W] int64 -> bool [B, N] on the device"""
    B, W = mask.shape
    sh = torch.arange(64, dtype=torch.int64, device=mask.device)
    return ((mask.view(B, W, 1) >> sh) & 1).view(B, W * 64)[:, :N].bool()


def check_full_set_is_informative(dev, oracle, synthetic, N, outside):
    key = ("info", N, outside)
    if key not in _scene:
        rays = full_rays(oracle, synthetic).to(dev)
        q, _ = query_points(rays, full_u(N).to(dev), tbins(N, dev), 0, 0, 0, N)
        live = T.live_of(q.view(10000, N, 6).cpu(), M.ball_cells(R129, BOUNDS, 1.0), R129, BOUNDS, outside)
        _scene[key] = M.require_informative(live, N, outside)
    return _scene[key]


def dense_backward(raw, ts, rays, g, B, N, dev):
    from nerf_simple_amd import _lib
    d = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().nerf_amd_volume_render_rays_backward(
        _lib.ptr(raw), _lib.ptr(ts), _lib.ptr(rays), *[_lib.ptr(x) for x in g], _lib.ptr(d), B, N, _lib.stream_ptr(dev)),
        "dense backward")
    return d


def masked_backward(raw_live, rays, args, m, g, B, N, dev, pad=8):
    """-> (d_raw_live [P', 4], the whole sentinel-padded buffer)"""
    from nerf_simple_amd import _lib
    jit, tb, flags, seed, rid = args
    P = raw_live.shape[0]
    buf = torch.full((P + 2 * pad, 4), SENTINEL, dtype=torch.float32, device=dev)
    out = buf[pad:pad + P]
    rc = _lib.lib().nerf_amd_volume_render_masked_backward(
        _lib.ptr(raw_live) if P else None, _lib.ptr(rays), _lib.ptr(jit), _lib.ptr(tb), flags, seed, rid, _lib.ptr(m.mask),
        _lib.ptr(m.offsets), *[_lib.ptr(x) for x in g], _lib.ptr(out) if P else None, B, N, _lib.stream_ptr(dev))
    _lib.check(rc, "masked backward")
    return out, buf


# ---- 1. the masked compositor's backward ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["u", "ts", "device_rng"])
def test_masked_backward_is_the_dense_backward_at_the_live_rows(dev, oracle, synthetic, mode):
    from nerf_simple_amd import _lib
    rays_all = full_rays(oracle, synthetic).to(dev)
    gen = torch.Generator().manual_seed(11)
    for N in NS:
        for outside in POLICIES:
            check_full_set_is_informative(dev, oracle, synthetic, N, outside)
        for B in BS:
            idx = torch.from_numpy(subset(B)).to(dev)
            rays = rays_all[idx].contiguous()
            u = full_u(N).to(dev)[idx].contiguous()
            tb = tbins(N, dev)
            if mode == "u":
                kw, args = dict(u=u), (u, tb, 0, 0, 0)
            elif mode == "ts":
                _, ts_in = query_points(rays, u, tb, 0, 0, 0, N)
                kw, args = dict(ts=ts_in), (ts_in, None, _lib.FLAG_TS_GIVEN, 0, 0)
            else:
                kw, args = dict(device_rng=True, seed=7, ray_id0=12345), (None, tb, _lib.FLAG_DEVICE_RNG, 7, 12345)
            _, ts = query_points(rays, *args, N)
            up = [torch.randn(s, generator=gen).to(dev) for s in ((B, 3), (B,), (B, N), (B,), (B, N))]
            combos = [tuple(x if j == i else None for j, x in enumerate(up)) for i in range(5)] + [tuple(up)]
            for outside in POLICIES:
                m = ball_grid(dev, outside).mark(rays, N, **kw)
                live = unpack_mask(m.mask, N)
                assert int(live.sum()) == m.live
                raw_live = torch.randn(m.live, 4, generator=gen)
                raw_live[:, 3] *= 2.0
                raw_live = raw_live.to(dev)
                raw = torch.tensor(T.DEAD_ROW, device=dev).expand(B, N, 4).clone()
                raw[live] = raw_live
                for ci, g in enumerate(combos):
                    d_ref = dense_backward(raw, ts, rays, g, B, N, dev)
                    got, buf = masked_backward(raw_live, rays, args, m, g, B, N, dev)
                    again, _ = masked_backward(raw_live, rays, args, m, g, B, N, dev)
                    where = (mode, N, B, outside, ci)
                    assert same(got, again), where                                   # two runs write the same bytes
                    assert (buf[:8] == SENTINEL).all() and (buf[8 + m.live:] == SENTINEL).all(), where
                    assert torch.isfinite(d_ref).all(), where
                    assert (d_ref[~live] == 0).all(), where                          # a dead sample receives nothing
                    assert same(got, d_ref[live]), where                             # the dense backward's live rows
                    if N == 1:
                        assert (got == 0).all(), where


def test_masked_backward_limits(dev, oracle, synthetic):
    from nerf_simple_amd import _lib
    from nerf_simple_amd.training import render_nerf_masked
    rays = full_rays(oracle, synthetic).to(dev)[torch.from_numpy(subset(63)).to(dev)].contiguous()
    B, N = 63, 513
    occ = ball_grid(dev, "live")
    u = torch.rand(B, N).to(dev)
    m = occ.mark(rays, N, u=u)                   # the forward stages serve N <= 768
    raw_live = torch.zeros((m.live, 4), device=dev)
    g = torch.zeros((B, 3), device=dev)
    d = torch.full((m.live, 4), SENTINEL, device=dev)
    rc = _lib.lib().nerf_amd_volume_render_masked_backward(
        _lib.ptr(raw_live), _lib.ptr(rays), _lib.ptr(u), _lib.ptr(tbins(N, dev)), 0, 0, 0, _lib.ptr(m.mask), _lib.ptr(m.offsets),
        _lib.ptr(g), None, None, None, None, _lib.ptr(d), B, N, _lib.stream_ptr(dev))
    assert rc == -2 and (d == SENTINEL).all()
    net = make_net(dev, "default")
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="512"):
        render_nerf_masked(rays, net, 513, occ)
    assert torch.equal(torch.get_rng_state(), state)
    # a grid with nothing live: P' = 0, NULL buffers, nothing launched that could write
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    dead = OccupancyGrid.from_mask(torch.zeros((8, 8, 8), dtype=torch.bool, device=dev), BOUNDS, outside="empty")
    m0 = dead.mark(rays, 64, u=u[:, :64].contiguous())
    assert m0.live == 0
    got, buf = masked_backward(torch.zeros((0, 4), device=dev), rays, (u[:, :64].contiguous(), tbins(64, dev), 0, 0, 0), m0,
                               (g, None, None, None, None), B, 64, dev)
    assert got.shape == (0, 4) and (buf == SENTINEL).all()


# ---- 2. the running density volume ------------------------------------------------------------------------------------------------
def decay_max_gpu(dev, state, sigma, decay):
    import ctypes
    from nerf_simple_amd import _lib
    s = torch.from_numpy(state).to(dev).contiguous()
    g = torch.from_numpy(sigma).to(dev).contiguous()
    _lib.check(_lib.lib().nerf_amd_occupancy_decay_max(_lib.ptr(s), _lib.ptr(g), ctypes.c_float(decay), s.numel(),
                                                       _lib.stream_ptr(dev)), "decay_max")
    return s.cpu().numpy()


def test_decay_max_against_the_model(dev):
    rng = np.random.default_rng(5)
    n = 100003                                     # not a multiple of the workgroup size
    state = (np.abs(rng.normal(size=n)) * 30).astype(np.float32)
    # exact part: sigma > 20 everywhere -- softplus is the identity, the decay product one float32 multiply
    big = (rng.random(n) * 60 + 20.001).astype(np.float32)
    for decay in (0.95, 0.5, 1.0, 0.0):
        got = decay_max_gpu(dev, state, big, decay)
        assert np.array_equal(got.view(np.uint32), T.decay_max(state, big, decay).view(np.uint32)), decay
    # NaN propagates from either side; infinities behave
    s2, g2 = state.copy(), big.copy()
    s2[3], g2[5], g2[7], s2[9] = np.nan, np.nan, np.inf, np.inf
    g2[11] = -np.inf
    got = decay_max_gpu(dev, s2, g2, 0.95)
    assert np.isnan(got[3]) and np.isnan(got[5]) and np.isnan(got).sum() == 2
    assert got[7] == np.inf and got[9] == np.inf and got[11] == np.float32(s2[11] * np.float32(0.95))
    # inexact part: general sigma, inside the fp32 rule against the float64 value
    sigma = (rng.normal(size=n) * 8).astype(np.float32)
    small = (np.abs(rng.normal(size=n)) * 2).astype(np.float32)
    for st in (state, small, np.zeros(n, np.float32)):
        got = decay_max_gpu(dev, st, sigma, 0.95)
        want, scale, bound = T.decay_max_bound(st, sigma, 0.95)
        err = float(np.abs(got.astype(np.float64) - want).max()) / scale
        print(f"decay_max: err {err:.3e} of bound {bound:.3e}")
        assert err <= bound and (got >= 0).all()


def test_update_writes_the_models_bits_and_cells_die_on_schedule(dev):
    from nerf_simple_amd.utils import mesh
    from nerf_simple_amd.utils.occupancy import TrainingOccupancyGrid
    from nerf_simple_amd.utils import synthetic
    R = (49, 53, 57)
    net = make_net(dev, "structured")
    occ = TrainingOccupancyGrid(R, BOUNDS, outside="empty", device=dev)
    assert occ.cell_fraction == 1.0 and occ.outside == "empty" and (occ.state == 0).all() and occ.cells().all()
    words_ptr = occ.words.data_ptr()
    sigma = mesh.density_grid(net, R, BOUNDS).cpu().numpy()
    level = float(np.percentile(sigma, 90))
    with pytest.raises(TypeError):
        occ.update(net)
    occ.update(net, level, decay=0.5, dilate=1)
    state = occ.state.cpu().numpy()
    want, scale, bound = T.decay_max_bound(np.zeros(R, np.float32), sigma, 0.5)
    assert float(np.abs(state - want).max()) / scale <= bound
    cells = T.cells_from_state(state, level, 1)
    assert occ.words.data_ptr() == words_ptr                                   # in place
    assert np.array_equal(occ.words.cpu().numpy().view(np.uint32), M.pack_bits(cells))
    assert abs(occ.cell_fraction - cells.mean()) < 1e-12 and 0 < occ.cell_fraction < 1
    # the network's sigma drops to nothing: a cell stays alive until decay^k of its hottest corner is <= softplus(level)
    # (decay 0.8 here, so that the schedule has several steps)
    sd = {k: v.clone() for k, v in synthetic.synthetic_state_dict(0, "structured").items()}
    sd["sigma_fc.0.bias"] -= 200.0
    gone = make_net(dev, "structured", sd=sd)
    assert float(mesh.density_grid(gone, R, BOUNDS).max()) < -100
    occ.update(gone, level, decay=0.8, dilate=0)                               # step k = 1
    state1 = occ.state.cpu().numpy()
    assert np.array_equal(state1.view(np.uint32), (state * np.float32(0.8)).astype(np.float32).view(np.uint32))
    i, j, k_ = np.unravel_index(np.argmax(state[:-1, :-1, :-1]), tuple(r - 1 for r in R))
    corners = state[i:i + 2, j:j + 2, k_:k_ + 2].reshape(-1)
    dies_at = max(T.steps_until_dead(c, 0.8, level) for c in corners)
    assert 2 <= dies_at < 40
    for step in range(1, dies_at + 1):
        if step > 1:
            occ.update(gone, level, decay=0.8, dilate=0)
        now = occ.state.cpu().numpy()
        assert np.array_equal(occ.words.cpu().numpy().view(np.uint32), M.pack_bits(T.cells_from_state(now, level, 0))), step
        assert bool(occ.cells()[i, j, k_]) == (step < dies_at), (step, dies_at)
    assert occ.updates == 1 + dies_at


# ---- 3. the step ----------------------------------------------------------------------------------------------------------------------
def step_inputs(oracle, synthetic, B, N):
    """the rays, targets and jitter of tests/test_gpu_training.py::test_fused_training_vs_oracle at this shape"""
    gen = torch.Generator().manual_seed(B * 1000 + N)
    pose = torch.from_numpy(oracle.spherical_to_pose(4, -30, 0)).float()
    side = int(np.ceil(np.sqrt(B)))
    rays = oracle.camera_rays(pose, [side, side, synthetic.focal_from_fov(side)])[:B].contiguous()
    gt = torch.rand(B, 3, generator=gen)
    u = torch.rand(B, N, generator=gen)
    return rays, gt, u


def masked_step(dev, kind, occ, rays, gt, u, N, **kw):
    from nerf_simple_amd.training import train_step
    net = make_net(dev, kind)
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    loss = train_step(net, opt, rays.to(dev), gt.to(dev), N, u=None if u is None else u.to(dev), occupancy=occ, **kw)
    return loss, {k: p.grad for k, p in net.named_parameters()}


@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("shape", [(576, 64), (37, 65), (64, 1)])
def test_all_live_grid_is_the_dense_points_mode_step(dev, oracle, synthetic, shape, kind):
    from nerf_simple_amd.training import mse_loss, nerf_forward_autograd, volume_render_autograd
    from nerf_simple_amd.utils.occupancy import TrainingOccupancyGrid
    B, N = shape
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    all_live = TrainingOccupancyGrid(17, BOUNDS, outside="live", device=dev)
    loss, grads = masked_step(dev, kind, all_live, rays, gt, u, N)
    assert all_live.last_stats == {"rays": B, "samples": B * N, "live": B * N, "network_launches": 1}
    # the dense points-mode composition on the same u
    net = make_net(dev, kind)
    q, ts = query_points(rays.to(dev), u.to(dev), tbins(N, dev), 0, 0, 0, N)
    raw = nerf_forward_autograd(net, q, "bf16").reshape(B, N, 4)
    dirs = q.view(B, N, 6)[:, 0, 3:6].contiguous()             # the unit directions the kernels formed
    rgb = volume_render_autograd(raw, ts, dirs)[0]
    want = mse_loss(rgb, gt.to(dev))
    want.backward()
    assert same(loss, want.detach()), (float(loss), float(want))
    # the run-to-run tolerance tests/test_gpu_training.py::test_ragged_training_ignores_garbage_beyond_P grants the dW products
    for k, p in net.named_parameters():
        scale = float(p.grad.abs().max())
        assert float((grads[k] - p.grad).abs().max()) <= 1e-5 * scale, (k, scale)


@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("outside", POLICIES)
@pytest.mark.parametrize("shape", [(576, 64), (37, 65)])
def test_ball_grid_step_within_the_model_bound(dev, oracle, synthetic, shape, outside, kind):
    B, N = shape
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    ts, q, dn = T.geometry(rays, u=u)
    live = T.live_of(q, M.ball_cells(R129, BOUNDS, 1.0), R129, BOUNDS, outside)
    frac, _, _ = M.require_informative(live, N, outside)
    assert 0.05 <= frac <= 0.95
    occ = ball_grid(dev, outside)
    loss, grads = masked_step(dev, kind, occ, rays, gt, u, N)
    assert occ.last_stats["live"] == int(live.sum()) and occ.last_stats["samples"] == B * N
    sd = synthetic.synthetic_state_dict(0, kind)

    def loss_of(forward, sdp, dtype):
        return T.masked_loss(forward, sdp, q, ts, dn, live, gt, dtype)
    loss64, report = T.model_bound_report(sd, loss_of, {k: g.float().cpu() for k, g in grads.items()})
    print(f"ball {shape} {outside} {kind}: live {frac:.3f}; loss {float(loss):.6g} vs float64 masked model {loss64:.6g} "
          f"(rel {abs(float(loss) - loss64) / abs(loss64):.2e})")
    worst = max(report, key=lambda k: report[k][0] / report[k][1])
    print(f"    worst tensor {worst}: err {report[worst][0]:.3e} of bound {report[worst][1]:.3e}")
    for k, (err, bound) in report.items():
        print(f"    {k:28s} {err:.3e} / {bound:.3e} = {err / bound:.3f}")
    assert abs(float(loss) - loss64) <= LOSS_RTOL[kind] * abs(loss64), (float(loss), loss64)
    bad = {k: v for k, v in report.items() if not v[0] <= v[1]}
    assert not bad, bad


def test_empty_batch(dev, oracle, synthetic):
    B, N = 576, 64
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    away = torch.cat([rays[:, :3], -rays[:, 3:]], 1).contiguous()       # the camera looks away from the grid
    _, q, _ = T.geometry(away, u=u)
    assert not T.live_of(q, np.ones((128, 128, 128), bool), R129, BOUNDS, "empty").any()
    occ = ball_grid(dev, "empty")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loss, grads = masked_step(dev, "default", occ, away, gt, u, N)
        torch.cuda.synchronize()
    assert occ.last_stats == {"rays": B, "samples": B * N, "live": 0, "network_launches": 0}
    want = float((gt.double() ** 2).mean())
    assert abs(float(loss) - want) <= 1e-6 * want, (float(loss), want)      # fp32 sum of 3 B squares
    for k, g in grads.items():
        assert g is not None and g.shape == synthetic.synthetic_state_dict(0, "default")[k].shape and (g == 0).all(), k
    # the device RNG and an explicit ts take the same route
    loss2, grads2 = masked_step(dev, "default", occ, away, gt, None, N, device_rng=True, seed=5)
    assert same(loss2, loss) and all(g is not None and (g == 0).all() for g in grads2.values())


def test_refusals_leave_the_generator_untouched(dev, oracle, synthetic):
    from nerf_simple_amd.training import render_nerf_masked, train_step
    from nerf_simple_amd.utils.nets import Nerf
    B, N = 37, 65
    rays, gt, _ = step_inputs(oracle, synthetic, B, N)
    rays, gt = rays.to(dev), gt.to(dev)
    occ = ball_grid(dev, "live")
    net = make_net(dev, "default")

    class Foreign:
        def forward(self, q):
            return torch.zeros(q.shape[0], 4, device=q.device)

    # every input is built BEFORE the generator is read: nn.Linear's initialisation draws from it
    fp32 = make_net(dev, "default", "fp32")
    small = Nerf(6, 4, 128).to(dev)
    grad_rays = rays.clone().requires_grad_(True)
    bad_u = torch.rand(B, N + 1, device=dev)
    cases = [
        ("rays that require grad", RuntimeError, lambda: render_nerf_masked(grad_rays, net, N, occ)),
        ("an fp32 module", RuntimeError, lambda: render_nerf_masked(rays, fp32, N, occ)),
        ("another network size", RuntimeError, lambda: render_nerf_masked(rays, small, N, occ)),
        ("a foreign net", RuntimeError, lambda: render_nerf_masked(rays, Foreign(), N, occ)),
        ("N > 512", RuntimeError, lambda: render_nerf_masked(rays, net, 513, occ)),
        ("not a grid", TypeError, lambda: render_nerf_masked(rays, net, N, object())),
        ("u of the wrong shape", RuntimeError, lambda: render_nerf_masked(rays, net, N, occ, u=bad_u)),
    ]
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    cases += [
        ("train_step, fp32 module", RuntimeError,
         lambda: train_step(fp32, torch.optim.SGD(fp32.parameters(), lr=0.0), rays, gt, N, occupancy=occ)),
        ("train_step, precision='fp32'", RuntimeError, lambda: train_step(net, opt, rays, gt, N, precision="fp32", occupancy=occ)),
        ("train_step, N > 512", RuntimeError, lambda: train_step(net, opt, rays, gt, 513, occupancy=occ)),
    ]
    for what, exc, call in cases:
        state = torch.get_rng_state()
        with pytest.raises(exc):
            call()
        assert torch.equal(torch.get_rng_state(), state), what
    # the inference renders keep refusing a grad-enabled call (tests/test_gpu_occupancy.py asserts the same)
    from nerf_simple_amd.utils.rendering import render_nerf
    with pytest.raises(RuntimeError, match="inference only"):
        render_nerf(rays, net, N, occupancy=occ)
    # ... and a call that goes through draws the reference's one torch.rand(B, N)
    state = torch.get_rng_state()
    render_nerf_masked(rays, net, N, occ)
    after = torch.get_rng_state()
    torch.set_rng_state(state)
    torch.rand(B, N)
    assert torch.equal(torch.get_rng_state(), after)


def test_outputs_and_gradients_of_all_five_outputs(dev, oracle, synthetic):
    """render_nerf_masked's 5-tuple equals the inference masked render's with the bf16 TRAINING forward underneath (dense
    alpha / w, zero at dead samples), and a loss on all five outputs reaches the parameters."""
    from nerf_simple_amd.training import nerf_forward_autograd, render_nerf_masked
    B, N = 576, 64
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    rays, u = rays.to(dev), u.to(dev)
    occ = ball_grid(dev, "empty")
    net = make_net(dev, "structured")
    outs = render_nerf_masked(rays, net, N, occ, u=u)
    m = occ.mark(rays, N, u=u, points=True)
    live = unpack_mask(m.mask, N)
    assert outs[2].shape == (B, N) and outs[4].shape == (B, N)
    assert (outs[2][~live] == 0).all() and (outs[4][~live] == 0).all() and (outs[4][live] != 0).any()
    raw = torch.tensor(T.DEAD_ROW, device=dev).expand(B, N, 4).clone()
    raw[live] = nerf_forward_autograd(net, m.points, "bf16").detach()
    from nerf_simple_amd.utils.rendering import volume_render
    q, ts = query_points(rays, u, tbins(N, dev), 0, 0, 0, N)
    want = volume_render(raw, ts, q.view(B, N, 6)[:, 0, 3:6].contiguous())
    for name, g, w in zip(("rgb", "disp", "alpha", "acc", "w"), outs, want):
        assert same(g.detach(), w), name
    has = outs[3] > 0
    (outs[0].sum() + outs[1][has].sum() + outs[2].sum() + outs[3].sum() + (outs[4] * ts).sum()).backward()
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and (p.grad != 0).any(), k


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------
# A sample at density softplus(LEVEL) has alpha = 1 - exp(-softplus(-1.75) * 4 / 64) = 1 - exp(-0.16022 * 0.0625) = 0.00996
# <= 0.01 at the step's sample spacing: what the grid drops is at most 1 % opaque per sample.
LEVEL = -1.75
STEPS, WARMUP, EVERY, BATCH, NS_E2E = 1500, 256, 16, 1024, 64
E2E_BOUNDS = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def scene_views(oracle, synthetic, side=32):
    cam = [side, side, synthetic.focal_from_fov(side)]
    train = [(30, 0), (30, 90), (30, 180), (30, 270), (-20, 45), (-20, 225), (60, 135)]
    rays = [oracle.camera_rays(torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, th, ph))).float(), cam) for th, ph in train]
    held = oracle.camera_rays(torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, 10, 300))).float(), cam)
    return torch.cat(rays).contiguous(), held.contiguous()


def train_run(dev, synthetic, rays, gt, held, held_gt, seed, masked):
    from nerf_simple_amd.training import img_psnr, lr_decay_factor, train_step
    from nerf_simple_amd.utils.occupancy import TrainingOccupancyGrid
    from nerf_simple_amd.utils.rendering import render_nerf
    net = make_net(dev, "default")
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    decay = lr_decay_factor(5e-4, 1e-4, STEPS)
    occ = TrainingOccupancyGrid(128, E2E_BOUNDS, outside="empty", device=dev) if masked else None
    gen = torch.Generator().manual_seed(1000 + seed)
    losses, fracs = [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(STEPS):
        ids = torch.randint(0, rays.shape[0], (BATCH,), generator=gen).to(dev)
        if masked and step >= WARMUP and step % EVERY == 0:
            occ.update(net, LEVEL)
        loss = train_step(net, opt, rays[ids], gt[ids], NS_E2E, decay=decay, device_rng=True, seed=seed * 100000 + step,
                          occupancy=occ)
        losses.append(loss)
        if masked:
            fracs.append(occ.last_stats["live"] / occ.last_stats["samples"])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / STEPS
    losses = torch.stack(losses).cpu().numpy()
    # A network trained through a grid is defined where the grid is live and nowhere else: outside="empty" keeps every
    # sample beyond the bounds from the loss from step 0 on, and a dropped cell stops receiving gradients.  The trained
    # model is the pair (net, grid), so the held-out view of a masked run is rendered through its grid, like any inference
    # render with that grid; the dense run is rendered densely.
    with torch.no_grad():
        rgb = render_nerf(held, net, 128, device_rng=True, seed=99, outputs=("rgb",), occupancy=occ)[0]
    psnr = float(img_psnr(held_gt.cpu(), rgb.cpu()))
    return dict(seed=seed, masked=masked, first_loss=float(losses[0]), final_loss=float(losses[-20:].mean()), psnr=psnr,
                ms_per_step=ms, live_last_100=max(fracs[-100:]) if masked else 1.0,
                cell_fraction=occ.cell_fraction if masked else 1.0)


def test_training_through_the_grid_end_to_end(dev, oracle, synthetic):
    rays, held = scene_views(oracle, synthetic)
    gt, held_gt = T.scene_targets(rays).to(dev), T.scene_targets(held).to(dev)
    rays, held = rays.to(dev), held.to(dev)
    runs = [train_run(dev, synthetic, rays, gt, held, held_gt, seed, masked) for masked in (False, True) for seed in (0, 1, 2)]
    for r in runs:
        print(json.dumps(r))
    out = os.environ.get("NERF_OCC_TRAIN_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(runs, f, indent=1)
    dense = [r for r in runs if not r["masked"]]
    masked = [r for r in runs if r["masked"]]
    for r in runs:
        assert r["final_loss"] < 0.05 * r["first_loss"], r                   # both kinds of run learn
    spread = max(r["psnr"] for r in dense) - min(r["psnr"] for r in dense)
    mean_d, mean_m = np.mean([r["psnr"] for r in dense]), np.mean([r["psnr"] for r in masked])
    print(f"held-out PSNR: dense {mean_d:.2f} dB (spread {spread:.2f}), masked {mean_m:.2f} dB")
    assert mean_m >= mean_d - spread, (mean_m, mean_d, spread)
    for r in masked:
        assert r["live_last_100"] <= 0.5, r                                  # the skipping was real
