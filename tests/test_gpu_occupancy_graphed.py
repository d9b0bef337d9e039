"""The graphed masked training step on the GPU (csrc/occupancy_graph.hip, training.GraphedMaskedTrainStep; DESIGN.md
section 14).  Yardsticks: tests/occupancy_graphed_model.py (the capacity semantics) on tests/occupancy_train_model.py.

Kernel level: the capped emit against nerf_amd_occupancy_points and the pad constant; the fused masked head against the
existing kernels run with mask_C / offsets_C built on the host (nerf_amd_volume_render_masked -> nerf_amd_mse_loss ->
nerf_amd_volume_render_masked_backward): rgb and d_raw bit for bit (every kernel of the chain runs
csrc/composite_backward_device.h), surplus rows exactly zero.  Step level: loss bit-equal to the eager masked step, gradients
within the dW products' run-to-run tolerance (1e-5 of the tensor's scale).  Trajectory: the criteria of tests/test_gpu_training.py::test_graphed_train_step_matches_eager.

Inputs: those of tests/test_gpu_occupancy_training.py (helpers copied).  Every capacity is derived from the live count the CPU
model gives for the case, never typed in.
"""
import warnings

import numpy as np
import pytest
import torch

import occupancy_graphed_model as G
import occupancy_model as M
import occupancy_train_model as T

pytestmark = pytest.mark.gpu

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R129 = (129, 129, 129)
BS = (1, 63, 1000)
NS = (1, 3, 64, 65, 128, 512)
POLICIES = ("empty", "live")
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


def step_inputs(oracle, synthetic, B, N):
    """the rays, targets and jitter of tests/test_gpu_training.py::test_fused_training_vs_oracle at this shape"""
    gen = torch.Generator().manual_seed(B * 1000 + N)
    pose = torch.from_numpy(oracle.spherical_to_pose(4, -30, 0)).float()
    side = int(np.ceil(np.sqrt(B)))
    rays = oracle.camera_rays(pose, [side, side, synthetic.focal_from_fov(side)])[:B].contiguous()
    gt = torch.rand(B, 3, generator=gen)
    u = torch.rand(B, N, generator=gen)
    return rays, gt, u


def check_full_set_is_informative(dev, oracle, synthetic, N, outside):
    key = ("info", N, outside)
    if key not in _scene:
        rays = full_rays(oracle, synthetic).to(dev)
        q, _ = query_points(rays, full_u(N).to(dev), tbins(N, dev), 0, 0, 0, N)
        live = T.live_of(q.view(10000, N, 6).cpu(), M.ball_cells(R129, BOUNDS, 1.0), R129, BOUNDS, outside)
        _scene[key] = M.require_informative(live, N, outside)
    return _scene[key]


def model_live(rays, args, N, outside, cells=None):
    """the CPU model's verdict (T.live_of) on the sample positions the kernels form for these jitter arguments"""
    q, _ = query_points(rays, *args, N)
    cells = M.ball_cells(R129, BOUNDS, 1.0) if cells is None else cells
    R = tuple(c + 1 for c in cells.shape)
    return T.live_of(q.view(rays.shape[0], N, 6).cpu(), cells, R, BOUNDS, outside)


def to_dev_mask(kept, dev):
    """bool [B, N] -> (mask words int64 [B, W], offsets int64 [B + 1]) on the device"""
    words = torch.from_numpy(M.mask_words(kept).view(np.int64).copy()).to(dev)
    return words, torch.from_numpy(M.offsets(kept)).to(dev)


def capped_emit(rays, args, mask, offsets, C, B, N, dev, pad=8):
    """-> (the whole sentinel-prefilled buffer [C + pad, 6], counts int64[2] as a list)"""
    from nerf_simple_amd import _lib
    jit, tb, flags, seed, rid = args
    buf = torch.full((C + pad, 6), SENTINEL, dtype=torch.float32, device=dev)
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().nerf_amd_occupancy_points_capped(
        _lib.ptr(rays), _lib.ptr(jit), _lib.ptr(tb), flags, seed, rid, _lib.ptr(mask), _lib.ptr(offsets), _lib.ptr(buf),
        _lib.ptr(counts), C, B, N, _lib.stream_ptr(dev)), "capped emit")
    return buf, counts.tolist()


def fused_head(raw, rays, args, mask, offsets, gt, C, B, N, dev, pad=8):
    """-> (rgb [B, 3], the whole sentinel-prefilled d_raw buffer [C + pad, 4])"""
    from nerf_simple_amd import _lib
    jit, tb, flags, seed, rid = args
    rgb = torch.full((B, 3), SENTINEL, dtype=torch.float32, device=dev)
    buf = torch.full((C + pad, 4), SENTINEL, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().nerf_amd_volume_render_masked_mse_backward(
        _lib.ptr(raw), _lib.ptr(rays), _lib.ptr(jit), _lib.ptr(tb), flags, seed, rid, _lib.ptr(mask), _lib.ptr(offsets),
        _lib.ptr(gt), _lib.ptr(rgb), _lib.ptr(buf), C, B, N, _lib.stream_ptr(dev)), "fused masked head")
    return rgb, buf


def reference_head(raw_kept, rays, args, mask_c, offsets_c, gt, B, N, dev):
    """the existing kernels under mask_C / offsets_C: masked compositor -> MSE gradient -> masked compositor backward"""
    from nerf_simple_amd import _lib
    lib = _lib.lib()
    jit, tb, flags, seed, rid = args
    K = raw_kept.shape[0]
    st = _lib.stream_ptr(dev)
    rgb = torch.empty((B, 3), dtype=torch.float32, device=dev)
    disp, acc = torch.empty(B, device=dev), torch.empty(B, device=dev)
    head = (_lib.ptr(raw_kept) if K else None, _lib.ptr(rays), _lib.ptr(jit), _lib.ptr(tb), flags, seed, rid, _lib.ptr(mask_c),
            _lib.ptr(offsets_c))
    _lib.check(lib.nerf_amd_volume_render_masked(*head, _lib.ptr(rgb), _lib.ptr(disp), None, _lib.ptr(acc), None, B, N, st),
               "masked compositor")
    loss, g = torch.empty((), device=dev), torch.empty((B, 3), device=dev)
    _lib.check(lib.nerf_amd_mse_loss(_lib.ptr(rgb), _lib.ptr(gt), _lib.ptr(loss), _lib.ptr(g), B * 3, st), "mse")
    d = torch.empty((K, 4), dtype=torch.float32, device=dev)
    _lib.check(lib.nerf_amd_volume_render_masked_backward(*head, _lib.ptr(g), None, None, None, None, _lib.ptr(d) if K else None,
                                                          B, N, st), "masked backward")
    return rgb, d


def jitter_args(mode, rays, u, N, dev):
    """(mark keywords, the reference kernels' jitter arguments, the new kernels' jitter arguments)"""
    from nerf_simple_amd import _lib
    tb = tbins(N, dev)
    if mode == "u":
        return dict(u=u), (u, tb, 0, 0, 0), (u, tb, 0, 0, 0)
    if mode == "ts":
        _, ts_in = query_points(rays, u, tb, 0, 0, 0, N)
        a = (ts_in, None, _lib.FLAG_TS_GIVEN, 0, 0)
        return dict(ts=ts_in), a, a
    # the new kernels take the seed as a graph node does: 4 + an offset of 3 read from device memory
    off = torch.tensor([3], dtype=torch.int64, device=dev)
    return (dict(device_rng=True, seed=7, ray_id0=12345), (None, tb, _lib.FLAG_DEVICE_RNG, 7, 12345),
            (off, tb, _lib.FLAG_DEVICE_RNG | _lib.FLAG_SEED_IN_MEMORY, 4, 12345))


# ---- 1. the two kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["u", "ts", "device_rng"])
def test_capped_emit_and_fused_head_against_the_existing_kernels(dev, oracle, synthetic, mode):
    rays_all = full_rays(oracle, synthetic).to(dev)
    gen = torch.Generator().manual_seed(13)
    pad_row = torch.tensor(G.PAD_POINT, device=dev)
    overflowed = 0
    for N in NS:
        for outside in POLICIES:
            check_full_set_is_informative(dev, oracle, synthetic, N, outside)
        for B in BS:
            idx = torch.from_numpy(subset(B)).to(dev)
            rays = rays_all[idx].contiguous()
            u = full_u(N).to(dev)[idx].contiguous()
            kw, ref_args, new_args = jitter_args(mode, rays, u, N, dev)
            gt = torch.rand(B, 3, generator=gen).to(dev)
            for outside in POLICIES:
                live = model_live(rays, ref_args, N, outside)
                total = int(live.sum())
                m = ball_grid(dev, outside).mark(rays, N, points=True, **kw)
                assert m.live == total, (mode, N, B, outside)
                raw_live = torch.randn(total, 4, generator=gen)
                raw_live[:, 3] *= 2.0
                raw_live = raw_live.to(dev)
                for C in G.capacities(total, B, N):
                    where = (mode, N, B, outside, C, total)
                    kept = min(total, C)
                    # -- capped emit
                    buf, counts = capped_emit(rays, new_args, m.mask, m.offsets, C, B, N, dev)
                    again, _ = capped_emit(rays, new_args, m.mask, m.offsets, C, B, N, dev)
                    assert same(buf, again), where                                    # two runs write the same bytes
                    assert counts == list(G.counts(live, C)), (where, counts)
                    assert same(buf[:kept], m.points[:kept]), where                   # the rows of nerf_amd_occupancy_points
                    assert same(buf[kept:C], pad_row.expand(C - kept, 6)), where      # the pad constant
                    assert (buf[C:] == SENTINEL).all(), where                         # nothing beyond row C
                    # -- fused head: raw[C, 4] with NaN in the surplus rows (never read)
                    kept_mask = G.mask_C(live, C)
                    mask_c, offsets_c = to_dev_mask(kept_mask, dev)
                    assert np.array_equal(offsets_c.cpu().numpy(), G.offsets_C(live, C)), where
                    raw = torch.full((C, 4), float("nan"), device=dev)
                    raw[:kept] = raw_live[:kept]
                    rgb_ref, d_ref = reference_head(raw_live[:kept].contiguous(), rays, ref_args, mask_c, offsets_c, gt, B, N, dev)
                    rgb, dbuf = fused_head(raw, rays, new_args, m.mask, m.offsets, gt, C, B, N, dev)
                    rgb2, dbuf2 = fused_head(raw, rays, new_args, m.mask, m.offsets, gt, C, B, N, dev)
                    assert same(rgb, rgb2) and same(dbuf, dbuf2), where
                    assert same(rgb, rgb_ref), where                                  # rgb bit for bit
                    assert (dbuf[kept:C] == 0).all() and (dbuf[C:] == SENTINEL).all(), where
                    got = dbuf[:kept]
                    assert torch.isfinite(d_ref).all() and torch.isfinite(got).all(), where
                    assert same(got, d_ref), where                                    # d_raw bit for bit
                    if N == 1:
                        assert (got == 0).all() and (rgb == 0).all(), where
                    no_kept = torch.from_numpy(kept_mask.sum(1) == 0).to(dev)
                    assert (rgb[no_kept] == 0).all(), where                           # a ray with nothing kept
                    overflowed += int(total > C)
    assert overflowed > 0


# ---- 2. the step -----------------------------------------------------------------------------------------------------------
def graphed_step(dev, kind, occ, rays, gt, u, N, C, **kw):
    """one graphed masked step with lr = 0 -> (loss, {name: gradient}, the stepper)"""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedMaskedTrainStep
    net = make_net(dev, kind)
    opt = FusedAdam(net, lr=0.0)
    stepper = GraphedMaskedTrainStep(net, opt, rays.shape[0], N, occ, C, **kw)
    loss = stepper.step(rays.to(dev), gt.to(dev), u=None if u is None else u.to(dev)).clone()
    return loss, {k: p.grad.clone() for k, p in net.named_parameters()}, stepper


def eager_step(dev, kind, occ, rays, gt, u, N, kept_mask=None, **kw):
    """the eager masked step with lr = 0; with ``kept_mask`` the existing autograd functions composed under mask_C"""
    from nerf_simple_amd import training
    net = make_net(dev, kind)
    rays, gt, u = rays.to(dev), gt.to(dev), u.to(dev)
    if kept_mask is None:
        opt = torch.optim.SGD(net.parameters(), lr=0.0)
        loss = training.train_step(net, opt, rays, gt, N, u=u, occupancy=occ, **kw)
    else:
        tb = tbins(N, dev)
        m = occ.mark(rays, N, u=u, points=True)
        K = int(kept_mask.sum())
        mask_c, offsets_c = to_dev_mask(kept_mask, dev)
        params = [p for _, p in net.named_parameters()]
        raw, _ = training._FusedDense.apply(net, None, None, None, 0, 0, 0, 1, m.points[:K].contiguous(), *params)
        rgb = training._MaskedVolumeRender.apply(raw.reshape(-1, 4), (rays, u, tb, 0, 0, 0, mask_c, offsets_c), rays.shape[0], N)[0]
        loss = training.mse_loss(rgb, gt)
        loss.backward()
        loss = loss.detach()
    return loss, {k: p.grad for k, p in net.named_parameters()}


def compare_gradients(got, want, where):
    # the run-to-run tolerance tests/test_gpu_training.py::test_ragged_training_ignores_garbage_beyond_P grants the dW products
    for k, g in want.items():
        scale = float(g.abs().max())
        assert float((got[k] - g).abs().max()) <= 1e-5 * scale, (where, k, scale)


STEP_CASES = [(576, 64, "empty"), (37, 65, "live"), (64, 1, "empty")]


@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("case", STEP_CASES)
def test_graphed_step_is_the_eager_masked_step(dev, oracle, synthetic, case, kind):
    B, N, outside = case
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    live = model_live(rays.to(dev), (u.to(dev), tbins(N, dev), 0, 0, 0), N, outside)
    M.require_informative(live, N, outside)
    total = int(live.sum())
    occ = ball_grid(dev, outside)
    want_loss, want = eager_step(dev, kind, occ, rays, gt, u, N)
    assert occ.last_stats["live"] == total
    for C in (total, min(-(-(total + 1) // 256) * 256, B * N)):                        # C >= P': exactly, and with surplus rows
        loss, grads, stepper = graphed_step(dev, kind, occ, rays, gt, u, N, C)
        assert stepper.counts() == {"step": 1, "samples": B * N, "live": total, "kept": total, "capacity": C}
        assert same(loss, want_loss), (case, kind, C, float(loss), float(want_loss))
        compare_gradients(grads, want, (case, kind, C))


@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("case", [(576, 64, "empty"), (37, 65, "empty")])
def test_overflowing_step_is_the_eager_step_under_mask_C(dev, oracle, synthetic, case, kind):
    B, N, outside = case
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    live = model_live(rays.to(dev), (u.to(dev), tbins(N, dev), 0, 0, 0), N, outside)
    M.require_informative(live, N, outside)
    total = int(live.sum())
    C = -(-total // 2)
    assert C not in set(M.offsets(live).tolist())                                      # the capacity cuts inside a ray
    kept_mask = G.mask_C(live, C)
    occ = ball_grid(dev, outside)
    want_loss, want = eager_step(dev, kind, occ, rays, gt, u, N, kept_mask=kept_mask)
    full_loss, _ = eager_step(dev, kind, occ, rays, gt, u, N)
    loss, grads, stepper = graphed_step(dev, kind, occ, rays, gt, u, N, C)
    assert stepper.counts() == {"step": 1, "samples": B * N, "live": total, "kept": C, "capacity": C}
    assert same(loss, want_loss), (case, kind, float(loss), float(want_loss))
    assert not same(loss, full_loss)                                                   # the dropped tail did matter
    compare_gradients(grads, want, (case, kind, C))


def test_all_dead_batch(dev, oracle, synthetic):
    B, N = 576, 64
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    away = torch.cat([rays[:, :3], -rays[:, 3:]], 1).contiguous()       # the camera looks away from the grid
    assert not model_live(away.to(dev), (u.to(dev), tbins(N, dev), 0, 0, 0), N, "empty").any()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loss, grads, stepper = graphed_step(dev, "default", ball_grid(dev, "empty"), away, gt, u, N, 0.25)
        assert stepper.capacity == B * N // 4
        assert stepper.counts() == {"step": 1, "samples": B * N, "live": 0, "kept": 0, "capacity": B * N // 4}
    want = float((gt.double() ** 2).mean())
    assert abs(float(loss) - want) <= 1e-6 * want, (float(loss), want)      # fp32 sum of 3 B squares
    for k, g in grads.items():
        assert (g == 0).all(), k


# ---- 3. trajectories ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_rng", [False, True])
def test_graphed_masked_trajectory_matches_eager(dev, oracle, synthetic, device_rng):
    """6 decayed FusedAdam steps, graphed against eager masked, under the criteria of
    tests/test_gpu_training.py::test_graphed_train_step_matches_eager; the six replays run with no host sync between them."""
    from nerf_simple_amd import _lib
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedMaskedTrainStep, lr_decay_factor, train_step
    B, N, seed = 576, 64, 40
    rays, gt, _ = step_inputs(oracle, synthetic, B, N)
    rays, gt = rays.to(dev), gt.to(dev)
    occ = ball_grid(dev, "empty")
    decay = lr_decay_factor(5e-4, 4e-4, 10)
    us = [torch.rand(B, N, generator=torch.Generator().manual_seed(100 + i)).to(dev) for i in range(6)]
    tb = tbins(N, dev)
    jit = [(None, tb, _lib.FLAG_DEVICE_RNG, seed + k, 0) for k in range(1, 7)] if device_rng else [(x, tb, 0, 0, 0) for x in us]
    totals = []
    for a in jit:
        live = model_live(rays, a, N, "empty")
        M.require_informative(live, N, "empty")
        totals.append(int(live.sum()))
    C = -(-(max(totals) + 1) // 256) * 256
    runs = []
    for graphed in (False, True):
        net = make_net(dev, "default")
        opt = FusedAdam(net, lr=5e-4)
        if graphed:
            stepper = GraphedMaskedTrainStep(net, opt, B, N, occ, C, device_rng=device_rng, seed=seed, check_every=2)
            torch.cuda.synchronize()
            with warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)                   # an overflow report would raise
                held = [stepper.step(rays, gt, u=None if device_rng else us[i], decay=decay).clone() for i in range(6)]
            losses = [float(x) for x in held]
            assert opt.step_count == 6 and stepper.counts()["live"] == totals[-1] and stepper.overflow_steps == 0
            assert stepper.last_stats["live"] == totals[stepper.last_stats["step"] - 1]
        else:
            kw = [dict(device_rng=True, seed=seed + k) for k in range(1, 7)] if device_rng else [dict(u=x) for x in us]
            losses = [float(train_step(net, opt, rays, gt, N, decay=decay, occupancy=occ, **kw[i])) for i in range(6)]
        assert abs(opt.param_groups[0]["lr"] - 5e-4 * decay ** 6) < 1e-12
        with torch.no_grad():
            probe = net(rays[:8].new_zeros(8, 6) + 0.1).cpu()
        runs.append((losses, torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu(), probe))
    (la, pa, qa), (lb, pb, qb) = runs
    print(f"trajectory device_rng={device_rng}: eager {la} graphed {lb}; capacity {C} for live counts {totals}")
    assert la[-1] < la[0] and lb[-1] < lb[0]
    np.testing.assert_allclose(la, lb, rtol=2e-3)
    d = (pa - pb).abs()
    assert float(d.max()) <= 6 * 5e-4 and float(d.mean()) <= 1e-5 and float((d > 1e-5).float().mean()) <= 0.06
    assert float((qa - qb).abs().max()) <= 2e-2 * max(1.0, float(qa.abs().max()))


def test_graphed_masked_step_selects_its_own_rays(dev, oracle, synthetic):
    """rays_from with device_rng=True: the next batch is selected on graph A's side branch, beside the dX chain.  Every
    replay trains on the oracle's batch for (seed, step) and, with lr = 0, gives the loss of the same stepper fed by hand
    and of the eager masked step on that batch, bit for bit."""
    from nerf_simple_amd import _lib
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedMaskedTrainStep, train_step
    from nerf_simple_amd.utils.dataload import RayGenerator
    rays_tab = full_rays(oracle, synthetic)
    gt_tab = torch.rand(rays_tab.shape[0], 3, generator=torch.Generator().manual_seed(21))
    n, B, N, seed = rays_tab.shape[0], 576, 64, 11
    rg = RayGenerator.from_tables(rays_tab, gt_tab, device=dev)
    occ = ball_grid(dev, "empty")
    C = B * N // 2
    net_a, net_b, net_e = (make_net(dev, "structured") for _ in range(3))
    auto = GraphedMaskedTrainStep(net_a, FusedAdam(net_a, lr=0.0), B, N, occ, C, device_rng=True, seed=seed, rays_from=rg)
    hand = GraphedMaskedTrainStep(net_b, FusedAdam(net_b, lr=0.0), B, N, occ, C, device_rng=True, seed=seed)
    eager_opt = torch.optim.SGD(net_e.parameters(), lr=0.0)
    for step in (1, 2, 3):
        la = auto.step().clone()
        want = torch.from_numpy(oracle.select_ids_counter(n, B, seed, step))
        assert torch.equal(auto.ray_ids.cpu(), want), step
        rays, gt = rays_tab[want].to(dev), gt_tab[want].to(dev)
        live = model_live(rays, (None, tbins(N, dev), _lib.FLAG_DEVICE_RNG, seed + step, 0), N, "empty")
        M.require_informative(live, N, "empty")
        assert int(live.sum()) <= C
        assert auto.counts()["live"] == int(live.sum()), step
        lb = hand.step(rays, gt).clone()
        le = train_step(net_e, eager_opt, rays, gt, N, device_rng=True, seed=seed + step, occupancy=occ)
        assert same(la, lb) and same(la, le), (step, float(la), float(lb), float(le))
    with pytest.raises(RuntimeError):
        auto.step(rays_tab[:B].to(dev), gt_tab[:B].to(dev))


# ---- 4. the grid and the reports ---------------------------------------------------------------------------------------
def test_grid_update_between_replays_and_replaced_words(dev, oracle, synthetic):
    from nerf_simple_amd.training import train_step
    from nerf_simple_amd.utils import mesh
    from nerf_simple_amd.utils.occupancy import TrainingOccupancyGrid
    B, N, R = 576, 64, (33, 33, 33)
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    occ = TrainingOccupancyGrid(R, BOUNDS, outside="empty", device=dev)
    args = (u.to(dev), tbins(N, dev), 0, 0, 0)
    before = model_live(rays.to(dev), args, N, "empty", cells=np.ones((32, 32, 32), bool))
    loss, _, stepper = graphed_step(dev, "structured", occ, rays, gt, u, N, 1.0)
    assert stepper.counts()["live"] == int(before.sum()) == stepper.counts()["kept"]
    # update() writes the bits in place: the next replay sees them
    sigma = mesh.density_grid(stepper.net, R, BOUNDS).cpu().numpy()
    level = float(np.percentile(sigma, 90))
    words_ptr = occ.words.data_ptr()
    occ.update(stepper.net, level, decay=0.5, dilate=1)
    assert occ.words.data_ptr() == words_ptr
    cells = T.cells_from_state(occ.state.cpu().numpy(), level, 1)
    assert np.array_equal(cells, occ.cells().cpu().numpy())
    after = model_live(rays.to(dev), args, N, "empty", cells=cells)
    frac = float(after.mean())
    print(f"grid update: live {int(before.sum())} -> {int(after.sum())} of {B * N} samples")
    assert 0.02 < frac < 0.6 and int(after.sum()) < int(before.sum())              # the update changed what is live, to neither extreme
    loss2 = stepper.step(rays.to(dev), gt.to(dev), u=u.to(dev)).clone()
    assert stepper.counts() == {"step": 2, "samples": B * N, "live": int(after.sum()), "kept": int(after.sum()), "capacity": B * N}
    want, _ = eager_step(dev, "structured", occ, rays, gt, u, N)               # lr = 0: the same weights
    assert same(loss2, want), (float(loss2), float(want))
    assert not same(loss2, loss)
    # a replaced words tensor is refused: its address is baked into the graph
    occ.words = occ.words.clone()
    with pytest.raises(RuntimeError, match="words"):
        stepper.step(rays.to(dev), gt.to(dev), u=u.to(dev))
    assert stepper.opt.step_count == 2


def test_overflow_is_reported(dev, oracle, synthetic):
    B, N = 576, 64
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    live = model_live(rays.to(dev), (u.to(dev), tbins(N, dev), 0, 0, 0), N, "empty")
    total = int(live.sum())
    C = -(-total // 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        _, _, stepper = graphed_step(dev, "default", ball_grid(dev, "empty"), rays, gt, u, N, C, check_every=1)
    assert stepper.last_stats is None and stepper.overflow_steps == 0          # nothing polled yet
    torch.cuda.synchronize()
    with pytest.warns(RuntimeWarning, match=rf"step 1 had {total} live samples for a capacity of {C} points"):
        stepper.step(rays.to(dev), gt.to(dev), u=u.to(dev))
    assert stepper.overflow_steps == 1
    assert stepper.last_stats == {"step": 1, "samples": B * N, "live": total, "kept": C, "capacity": C}
    with pytest.warns(RuntimeWarning, match="step 2"):
        now = stepper.counts()                                                 # delivers the pending report, then reads
    assert now == {"step": 2, "samples": B * N, "live": total, "kept": C, "capacity": C}
    assert stepper.overflow_steps == 2 and stepper.last_stats["step"] == 2
    # a capacity that holds the batch stays silent
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        _, _, quiet = graphed_step(dev, "default", ball_grid(dev, "empty"), rays, gt, u, N, total, check_every=1)
        torch.cuda.synchronize()
        quiet.step(rays.to(dev), gt.to(dev), u=u.to(dev))
        assert quiet.counts()["kept"] == total
    assert quiet.overflow_steps == 0 and quiet.last_stats["live"] == total


def test_refusals_leave_the_generator_untouched(dev, oracle, synthetic):
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedMaskedTrainStep
    from nerf_simple_amd.utils.nets import Nerf
    B, N = 37, 65
    occ = ball_grid(dev, "live")
    net = make_net(dev, "default")
    opt = FusedAdam(net, lr=5e-4)

    class Foreign:
        precision = "bf16"

        def forward(self, q):
            return torch.zeros(q.shape[0], 4, device=q.device)

    # every input is built BEFORE the generator is read: nn.Linear's initialisation draws from it
    fp32 = make_net(dev, "default", "fp32")
    small = Nerf(6, 4, 128).to(dev)
    other = FusedAdam(make_net(dev, "default"), lr=5e-4)
    cases = [
        ("storage='e4m3'", ValueError, lambda: GraphedMaskedTrainStep(net, opt, B, N, occ, 0.5, storage="e4m3")),
        ("buckets=2", ValueError, lambda: GraphedMaskedTrainStep(net, opt, B, N, occ, 0.5, buckets=2)),
        ("N > 512", RuntimeError, lambda: GraphedMaskedTrainStep(net, opt, B, 513, occ, 0.5)),
        ("an fp32 module", RuntimeError, lambda: GraphedMaskedTrainStep(fp32, None, B, N, occ, 0.5)),
        ("another network size", RuntimeError, lambda: GraphedMaskedTrainStep(small, None, B, N, occ, 0.5)),
        ("a foreign net", RuntimeError, lambda: GraphedMaskedTrainStep(Foreign(), None, B, N, occ, 0.5)),
        ("not a grid", TypeError, lambda: GraphedMaskedTrainStep(net, opt, B, N, object(), 0.5)),
        ("another module's optimizer", RuntimeError, lambda: GraphedMaskedTrainStep(net, other, B, N, occ, 0.5)),
        ("no capacity", TypeError, lambda: GraphedMaskedTrainStep(net, opt, B, N, occ)),
        ("capacity 0", ValueError, lambda: GraphedMaskedTrainStep(net, opt, B, N, occ, 0)),
        ("capacity beyond B N", ValueError, lambda: GraphedMaskedTrainStep(net, opt, B, N, occ, B * N + 1)),
        ("a fraction beyond 1", ValueError, lambda: GraphedMaskedTrainStep(net, opt, B, N, occ, 1.5)),
        ("a capacity that is no number", TypeError, lambda: GraphedMaskedTrainStep(net, opt, B, N, occ, "half")),
    ]
    for what, exc, call in cases:
        state = torch.get_rng_state()
        with pytest.raises(exc):
            call()
        assert torch.equal(torch.get_rng_state(), state), what
    # the optimizer and the module are still usable: a stepper that is accepted trains
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    stepper = GraphedMaskedTrainStep(net, opt, B, N, occ, 1.0)
    before = opt.flat.clone()
    stepper.step(rays.to(dev), gt.to(dev), u=u.to(dev))
    torch.cuda.synchronize()
    assert not torch.equal(opt.flat, before) and opt.step_count == 1
