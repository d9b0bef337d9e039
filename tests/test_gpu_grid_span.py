"""The grid span on the GPU (csrc/grid_span.hip, utils/box.py ``GridSpan``, training.GraphedBoxTrainStep /
GraphedMaskedBoxTrainStep with a span).  Yardstick: tests/grid_span_model.py -- the definition op for op
in fp32, which the kernel must equal BIT FOR BIT -- on the scene box's case table and a subset of the full rays, against the
ball grid (K = 256), a hand-made anisotropic grid (K = 64), a 33^3 grid at K = 192 (j / K inexact) and an all-dead grid.

Kernel level: every jitter mode against the model; the invariants; poisoned guards behind every output; NULL span / hit; two
runs, the same bytes.  Render level: ``box=span`` is the ``ts=`` path on ``span.positions`` bit for bit, through every
precision, the grid (both policies) and ray termination; ``render_view`` and ``evaluate`` likewise.  Step level, lr = 0: the
eager step is the step on the placed positions; the two graphed steppers are the eager step with seed + k (losses bit for
bit, gradients within the dW products' run-to-run tolerance), follow ``occ.update()`` between replays and refuse a replaced
``words``.  Shapes, rays and helpers: tests/test_gpu_box.py and tests/test_gpu_occupancy_graphed.py."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import box_model as BM
import grid_span_model as M
import occupancy_graphed_model as G
import occupancy_model as OM
import test_gpu_occupancy_graphed as OG
from test_gpu_occupancy_graphed import ball_grid, compare_gradients, make_net, same, step_inputs, to_dev_mask

pytestmark = pytest.mark.gpu

BS = (37, 576)
NS = (1, 2, 63, 64, 65, 130)
SENTINEL = OG.SENTINEL
PAD = 16
STD, LAM = 0.5, 0.5
TN, TF = BM.TN, BM.TF
GRIDS = {"ball": (M.ball, 256), "hand_made": (M.hand_made, 64), "ball33": (M.ball33, 192), "all_dead": (M.all_dead, 64)}
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def grid_pair(dev, name):
    """(the model's grid, the same cells as an OccupancyGrid on the device, K)"""
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    if name not in _cache:
        make, K = GRIDS[name]
        g = make()
        _cache[name] = (g, OccupancyGrid.from_mask(torch.from_numpy(g.cells).to(dev), g.bounds, outside="empty"), K)
    return _cache[name]


def launch(dev, occ, K, rays, jit, flags, seed, rid, N, *, span=True, hit=True, tn=TN, tf=TF):
    """nerf_amd_span_positions itself on pre-poisoned buffers with a guard of PAD elements behind each -> (ts, span, hit) on
    the CPU; the guards must come back untouched."""
    from nerf_simple_amd import _lib as L
    from nerf_simple_amd.utils.rendering import _tbins
    B = rays.shape[0]
    ts = torch.full((B * N + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    sp = torch.full((2 * B + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    ht = torch.full((B + PAD,), -7, dtype=torch.int32, device=dev)
    tb = None if flags & L.FLAG_TS_GIVEN else _tbins(0, 1, N, dev)
    jp = L.ptr(jit) if (jit is None or torch.is_tensor(jit)) else jit
    rc = L.lib().nerf_amd_span_positions(L.ptr(rays), jp, L.ptr(tb), flags, seed, rid, L.ptr(occ.words), *occ.resolution, f3(occ.lo),
                                         f3(occ.bounds[1]), f3(occ.inv_step), K, tn, tf, L.ptr(ts),
                                         L.ptr(sp) if span else None, L.ptr(ht) if hit else None, B, N, L.stream_ptr(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((ts[B * N:] == SENTINEL).all()) and bool((sp[2 * B:] == SENTINEL).all()) and bool((ht[B:] == -7).all())
    if not span:
        assert bool((sp == SENTINEL).all())
    if not hit:
        assert bool((ht == -7).all())
    return ts[:B * N].view(B, N).cpu(), sp[:2 * B].view(B, 2).cpu(), ht[:B].cpu()


def same3(got, want):
    return all(same(g, w) for g, w in zip(got, want))


def check_invariants(ts, span, hit, all_dead=False):
    assert not torch.isnan(ts).any() and not torch.isnan(span).any()
    assert bool(((ts >= span[:, :1]) & (ts <= span[:, 1:])).all())
    assert bool((ts[:, 1:] >= ts[:, :-1]).all())
    miss = hit == 0
    assert bool(((hit == 0) | (hit == 1)).all()) and bool(miss.any()) and bool(miss.all()) == all_dead
    assert bool((span[miss] == torch.tensor([TN, TF])).all())
    assert bool(((span[~miss, 0] >= TN) & (span[~miss, 0] < span[~miss, 1]) & (span[~miss, 1] <= TF)).all())


def ray_sets(oracle, synthetic, B):
    """The scene box's case table (axis-parallel, NaN, misses, origin inside) and B of the 10,000 full rays."""
    return {"table": BM.case_table(B)[0], "full": OG.full_rays(oracle, synthetic)[torch.from_numpy(OG.subset(B))].contiguous()}


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_kernel_is_the_model(dev, oracle, synthetic, B, N):
    from nerf_simple_amd import _lib as L
    from nerf_simple_amd.utils.rendering import _query_points, _tbins
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(1000 * B + N))
    c = BM.unit_positions(u, N)
    seed, rid, off = 77 + N, 5 * B, 3
    mem = torch.tensor([off], dtype=torch.int64, device=dev)
    hits = {}
    for which, rays in ray_sets(oracle, synthetic, B).items():
        rd = rays.to(dev)
        # the counter RNG's unit positions are nerf_amd_query_points' on unit bins, same seed, same ray ids
        c_rng = _query_points(rd, None, _tbins(0, 1, N, dev), L.FLAG_DEVICE_RNG, seed, rid, N)[1].cpu()
        assert bool((c_rng >= 0).all()) and bool((c_rng <= 1).all()) and not same(c_rng, c)
        for name in GRIDS:
            g, occ, K = grid_pair(dev, name)
            where = (which, name, B, N)
            want = M.positions(rays, g, K, TN, TF, c)
            got = launch(dev, occ, K, rd, u.to(dev), 0, 0, 0, N)                                   # explicit u
            assert same3(got, want), where
            if which == "table" or name == "all_dead":
                check_invariants(*got, all_dead=name == "all_dead")
            hits[where[:2]] = int(got[2].sum())
            assert same3(launch(dev, occ, K, rd, c.to(dev), L.FLAG_TS_GIVEN, 0, 0, N), want), where           # given positions
            want_rng = M.positions(rays, g, K, TN, TF, c_rng)
            got_rng = launch(dev, occ, K, rd, None, L.FLAG_DEVICE_RNG, seed, rid, N)               # the counter RNG
            assert same3(got_rng, want_rng), where
            # the seed in memory: the bare seed plus the offset
            got_mem = launch(dev, occ, K, rd, ctypes.c_void_p(mem.data_ptr()), L.FLAG_DEVICE_RNG | L.FLAG_SEED_IN_MEMORY, seed - off,
                             rid, N)
            assert same3(got_mem, got_rng), where
            # NULL span / hit are skipped, ts is what it was; two runs write the same bytes
            assert same(launch(dev, occ, K, rd, u.to(dev), 0, 0, 0, N, span=False, hit=False)[0], got[0]), where
            assert same3(launch(dev, occ, K, rd, u.to(dev), 0, 0, 0, N), got), where
        assert not same(launch(dev, occ, K, rd, None, L.FLAG_DEVICE_RNG, seed, rid + 1, N)[0], got_rng[0])    # the ray ids matter
    print(f"B={B} N={N}: rays with a live cell {hits}")
    assert all(v == 0 for k, v in hits.items() if k[1] == "all_dead")
    assert all(v > 0 for k, v in hits.items() if k[1] != "all_dead")


def test_hand_made_grid_and_other_intervals(dev):
    """The ray through the two cells with a gap between them gets ONE interval over both; a corner cell on the grid's edge and
    a NaN ray are ordinary inputs; another [tn, tf] clips as the model says."""
    g, occ, K = grid_pair(dev, "hand_made")
    nan = float("nan")
    rays = torch.tensor([M.gap_ray(),
                         [4.0, 2.0, -3.0, -0.5, -0.25, 0.4],            # into the corner cell (7, 3, 0) from outside the grid
                         [1.9, 0.9, -1.4, 0.0, 0.0, 0.0],               # a zero direction inside the corner cell
                         [nan, 0.0, 0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, nan, nan, nan],
                         [-5.0, 0.25, -0.25, 1.0, 0.0, 0.0]], dtype=torch.float32)                 # the interior cell (3, 2, 2)
    N = 8
    c = BM.unit_positions(torch.rand(rays.shape[0], N, generator=torch.Generator().manual_seed(3)), N)
    for tn, tf in ((TN, TF), (0.5, 9.0), (3.6, 5.75)):
        want = M.positions(rays, g, K, tn, tf, c)
        got = launch(dev, occ, K, rays.to(dev), c.to(dev), 1, 0, 0, N, tn=tn, tf=tf)
        assert same3(got, want), (tn, tf)
    ts, span, hit = launch(dev, occ, K, rays.to(dev), c.to(dev), 1, 0, 0, N)
    assert hit.tolist() == [1, 1, 1, 0, 0, 1]
    assert span[0].tolist() == [3.0 + 10 * 3.0 / 64, 6.0]               # from cell 1's segment to cell 5's end at tf: the gap stays inside
    assert span[2].tolist() == [TN, TF] and 4.4 < float(span[5, 0]) <= 4.5 and 5.0 <= float(span[5, 1]) < 5.1


def test_empty_problem_and_python_call(dev, oracle, synthetic):
    from nerf_simple_amd import _lib as L
    from nerf_simple_amd.utils.box import GridSpan
    g, occ, K = grid_pair(dev, "ball")
    one = torch.zeros(8, device=dev)
    assert L.lib().nerf_amd_span_positions(None, L.ptr(one), L.ptr(one), 0, 0, 0, L.ptr(occ.words), *occ.resolution, f3(occ.lo),
                                           f3(occ.bounds[1]), f3(occ.inv_step), K, 2.0, 6.0, None, None, None, 0, 64,
                                           L.stream_ptr(dev)) == 0
    B, N = 576, 65
    rays = ray_sets(oracle, synthetic, B)["full"]
    rd = rays.to(dev)
    s = GridSpan(occ)
    assert s.probes == K == 256
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(4))
    want = M.positions(rays, g, K, TN, TF, BM.unit_positions(u, N))
    ts, span, hit = s.positions(rd, N, u=u.to(dev), return_span=True)
    assert same3((ts.cpu(), span.cpu(), hit.cpu()), want) and hit.dtype == torch.int32
    assert same(s.positions(rd, N, u=u.to(dev)), ts) and not ts.requires_grad
    assert same(s.positions(rd.clone().requires_grad_(True), N, u=u.to(dev)), ts)
    assert same(GridSpan(occ, 512).positions(rd, N, u=u.to(dev)).cpu(), M.positions(rays, g, 512, TN, TF, BM.unit_positions(u, N))[0])
    # the default jitter is the reference's one torch.rand(B, N), and leaves the generator where the reference leaves it
    torch.manual_seed(11)
    got = s.positions(rd, N)
    state = torch.get_rng_state()
    torch.manual_seed(11)
    u_ref = torch.rand(B, N)
    assert torch.equal(torch.get_rng_state(), state)
    assert same(got.cpu(), M.positions(rays, g, K, TN, TF, BM.unit_positions(u_ref, N))[0])
    # a refused call leaves the generator where it was
    for call in (lambda: s.positions(rd, 769), lambda: s.positions(rd, N, tn=6, tf=2), lambda: s.positions(rd, N, u=u.to(dev)[:, :3]),
                 lambda: s.positions(rd[:, :5], N)):
        with pytest.raises((RuntimeError, ValueError)):
            call()
    assert torch.equal(torch.get_rng_state(), state)
    with pytest.raises(ValueError, match="outside='empty'"):
        GridSpan(ball_grid(dev, "live"))


# ---- the renders -----------------------------------------------------------------------------------------------------------------
def ball_span(dev):
    from nerf_simple_amd.utils.box import GridSpan
    return GridSpan(ball_grid(dev, "empty"))


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_render_nerf_span_is_its_ts_path(dev, oracle, synthetic, precision):
    from nerf_simple_amd.utils.occupancy import EarlyTermination
    from nerf_simple_amd.utils.rendering import render_nerf
    B, N = 576, 64
    rays, _, u = (x.to(dev) for x in step_inputs(oracle, synthetic, B, N))
    net = make_net(dev, "structured", precision)
    s = ball_span(dev)
    ts = s.positions(rays, N, u=u)
    with torch.no_grad():
        got, want = render_nerf(rays, net, N, box=s, u=u), render_nerf(rays, net, N, ts=ts)
        assert all(same(g, w) for g, w in zip(got, want)), precision
        assert not same(got[0], render_nerf(rays, net, N, u=u)[0])                                 # the span did matter
        kw = dict(device_rng=True, seed=9, ray_id0=100)
        got, want = render_nerf(rays, net, N, box=s, **kw), render_nerf(rays, net, N, ts=s.positions(rays, N, **kw))
        assert all(same(g, w) for g, w in zip(got, want)), precision
        for outside in OG.POLICIES:                                                                # any grid, either policy
            occ = ball_grid(dev, outside)
            got, want = render_nerf(rays, net, N, box=s, u=u, occupancy=occ), render_nerf(rays, net, N, ts=ts, occupancy=occ)
            assert all(same(g, w) for g, w in zip(got, want)), (precision, outside)
        other = grid_pair(dev, "ball33")[1]                                                        # not the span's own grid
        got, want = render_nerf(rays, net, N, box=s, u=u, occupancy=other), render_nerf(rays, net, N, ts=ts, occupancy=other)
        assert all(same(g, w) for g, w in zip(got, want)), precision
        term, occ = EarlyTermination(1e-3, 32), ball_grid(dev, "empty")
        for path in (dict(terminate=term), dict(terminate=term, occupancy=occ)):
            got, want = render_nerf(rays, net, N, box=s, u=u, **path), render_nerf(rays, net, N, ts=ts, **path)
            assert all(same(g, w) for g, w in zip(got, want)), (precision, sorted(path))
        # the default jitter: one reference draw, consumed as the reference consumes it
        torch.manual_seed(5)
        got = render_nerf(rays, net, N, box=s)
        state = torch.get_rng_state()
        torch.manual_seed(5)
        want = render_nerf(rays, net, N, ts=s.positions(rays, N, u=torch.rand(B, N).to(dev)))
        assert torch.equal(torch.get_rng_state(), state) and all(same(g, w) for g, w in zip(got, want))


def test_render_view_and_evaluate(dev, oracle, synthetic):
    from nerf_simple_amd.utils import metrics as MT
    from nerf_simple_amd.utils.dataload import RayGenerator
    from nerf_simple_amd.utils.rendering import generate_rays, render_nerf, render_view
    S, N = 24, 64
    cam = [S, S, synthetic.focal_from_fov(S)]
    pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, -30, 0))).float()
    net = make_net(dev, "structured", "fp16")
    s = ball_span(dev)
    u = torch.rand(S * S, N, generator=torch.Generator().manual_seed(2)).to(dev)
    rays = generate_rays(pose, cam, dev)

    def composed(ts, **kw):
        rgb, disp, _, _, _ = render_nerf(rays, net, N, ts=ts, **kw)
        return torch.cat([rgb.clamp(0., 1.), disp[:, None]], dim=1)

    with torch.no_grad():
        ts = s.positions(rays, N, u=u)
        assert same(render_view(net, pose, cam, N=N, u=u, box=s), composed(ts))
        assert not same(render_view(net, pose, cam, N=N, u=u, box=s), render_view(net, pose, cam, N=N, u=u))
        for outside in OG.POLICIES:
            occ = ball_grid(dev, outside)
            assert same(render_view(net, pose, cam, N=N, u=u, box=s, occupancy=occ), composed(ts, occupancy=occ)), outside
        bg = torch.tensor([0.25, 0.5, 0.75], device=dev)
        assert same(render_view(net, pose, cam, N=N, u=u, box=s, background=bg), composed(ts, background=bg))
        # the counter RNG is keyed by global pixel id: a pixel range is that range of the whole view
        whole = render_view(net, pose, cam, N=N, device_rng=True, seed=4, box=s)
        assert same(whole, composed(s.positions(rays, N, device_rng=True, seed=4)))
        assert same(render_view(net, pose, cam, N=N, device_rng=True, seed=4, box=s, ray0=100, n_rays=200), whole[100:300])
    # evaluate passes box= on to render_view
    gen = np.random.default_rng(5)
    samples = {"val": [{"img": gen.random((16, 16, 3), dtype=np.float32), "transform": oracle.spherical_to_pose(4, -30, 40.0 * i)}
                       for i in range(2)]}
    cam16 = [16, 16, synthetic.focal_from_fov(16)]
    rg = RayGenerator.from_samples(samples, cam16, dev)
    out = MT.evaluate(net, rg, "val", N=16, device_rng=True, box=s)
    by_hand = MT.evaluate(net, rg, "val", render=lambda p: render_view(net, p, cam16, N=16, device_rng=True, box=s))
    assert out == by_hand and out["views"] == 2 and out != MT.evaluate(net, rg, "val", N=16, device_rng=True)


def unpack(mask, N):
    """mask words int64 [B, W] -> bool [B, N] (numpy)"""
    bit = (mask[:, :, None] >> torch.arange(64, device=mask.device)) & 1
    return bit.reshape(mask.shape[0], -1)[:, :N].bool().cpu().numpy()


def test_the_span_raises_the_live_count(dev, oracle, synthetic):
    """The mark kernel's own count on the 10,000 full rays, N = 64: span > live cells' box > plain, at least 0.9 N live samples
    on a ray that hits, none on a ray that does not."""
    from nerf_simple_amd.utils.box import SceneBox
    N = 64
    rays = OG.full_rays(oracle, synthetic).to(dev)
    u = OG.full_u(N).to(dev)
    occ = ball_grid(dev, "empty")
    s = ball_span(dev)
    ts, span, hit = s.positions(rays, N, u=u, return_span=True)
    plain, boxed = occ.mark(rays, N, u=u), occ.mark(rays, N, ts=SceneBox.from_occupancy(occ).positions(rays, N, u=u))
    spanned = occ.mark(rays, N, ts=ts)
    per_ray = (spanned.offsets[1:] - spanned.offsets[:-1]).cpu()
    miss = hit.cpu() == 0
    print(f"live {plain.live} (plain) -> {boxed.live} (box) -> {spanned.live} (span) of {rays.shape[0] * N}; "
          f"{int((~miss).sum())} rays hit; live per hit ray {spanned.live / int((~miss).sum()):.1f}")
    assert spanned.live > boxed.live > plain.live
    assert spanned.live >= 0.9 * N * int((~miss).sum())
    assert bool(miss.any()) and not bool(per_ray[miss].any())
    plain_per_ray = (plain.offsets[1:] - plain.offsets[:-1]).cpu()
    assert not bool(plain_per_ray[miss].any())                                   # conservative: a miss had no live sample before


# ---- the steps, lr = 0 -------------------------------------------------------------------------------------------------------------
def grads_of(net):
    return {k: p.grad.clone() for k, p in net.named_parameters()}


def test_eager_step_is_the_step_on_the_placed_positions(dev, oracle, synthetic):
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils.rendering import render_nerf
    B, N = 576, 64
    rays, gt, u = (x.to(dev) for x in step_inputs(oracle, synthetic, B, N))
    s = ball_span(dev)
    ts = s.positions(rays, N, u=u)
    for occ in (None, ball_grid(dev, "empty")):
        net, twin = make_net(dev, "structured"), make_net(dev, "structured")
        okw = {} if occ is None else dict(occupancy=occ)
        loss = T.train_step(net, torch.optim.SGD(net.parameters(), lr=0.0), rays, gt, N, u=u, box=s, **okw)
        rgb = (render_nerf(rays, twin, N, ts=ts) if occ is None else T.render_nerf_masked(rays, twin, N, occ, ts=ts))[0]
        want = T.mse_loss(rgb, gt)
        assert same(loss, want.detach()), (occ is None, float(loss), float(want))
        want.backward()
        compare_gradients(grads_of(net), grads_of(twin), ("eager", occ is None))
        other = make_net(dev, "structured")
        plain = T.train_step(other, torch.optim.SGD(other.parameters(), lr=0.0), rays, gt, N, u=u, **okw)
        assert not same(loss, plain)
    # the three controls through the grid: the torch expression on the masked render of the placed positions; the distortion
    # term keeps the global tf
    occ = ball_grid(dev, "empty")
    bg = torch.rand(B, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    c = T.Controls(background=bg, sigma_noise=STD, noise_seed=41, distortion=LAM)
    net, twin = make_net(dev, "default"), make_net(dev, "default")
    loss = T.train_step(net, torch.optim.SGD(net.parameters(), lr=0.0), rays, gt, N, u=u, ray_id0=9, occupancy=occ, box=s, controls=c)
    rgb, _, _, acc, w = T.render_nerf_masked(rays, twin, N, occ, ts=ts, ray_id0=9, controls=T.Controls(sigma_noise=STD, noise_seed=41))
    assert same(w.ts, ts)
    term = T._distortion_term(w, w.ts, LAM, 2, 6)
    want = T.mse_loss(rgb + (1 - acc)[:, None] * bg, gt) + term
    assert same(loss, want.detach()) and same(loss.distortion, term.detach()) and float(term.detach()) > 0


@pytest.mark.parametrize("mode", ["u", "device_rng"])
def test_graphed_span_step_is_the_eager_step(dev, oracle, synthetic, mode):
    from nerf_simple_amd import training as T
    from nerf_simple_amd.optim import FusedAdam
    B, N, seed, rid = 576, 64, 40, 3
    rays, gt, _ = (x.to(dev) for x in step_inputs(oracle, synthetic, B, N))
    us = [torch.rand(B, N, generator=torch.Generator().manual_seed(100 + k)).to(dev) for k in range(3)]
    s = ball_span(dev)
    rng = mode == "device_rng"
    net, twin = make_net(dev, "structured"), make_net(dev, "structured")
    stepper = T.GraphedBoxTrainStep(net, FusedAdam(net, lr=0.0), B, N, s, device_rng=rng, seed=seed, ray_id0=rid, check_every=2)
    opt_twin = torch.optim.SGD(twin.parameters(), lr=0.0)
    seen = []
    for k in (1, 2, 3):
        ekw = dict(device_rng=True, seed=seed + k, ray_id0=rid) if rng else dict(u=us[k - 1])
        loss = stepper.step(rays, gt, u=None if rng else us[k - 1]).clone()
        want = T.train_step(twin, opt_twin, rays, gt, N, box=s, **ekw)
        assert same(loss, want), (mode, k, float(loss), float(want))
        assert same(stepper.ts_box, s.positions(rays, N, **ekw)) and same(stepper.ts, stepper.ts_box), (mode, k)
        if k == 1:
            compare_gradients(grads_of(net), grads_of(twin), (mode, k))
        seen.append(float(loss))
    assert len(set(seen)) == 3                                                    # the jitter moved with the step
    assert not same(loss, T.train_step(twin, opt_twin, rays, gt, N, **ekw))       # the span did matter


def live_of(dev, occ, rays, N, ts):
    m = occ.mark(rays, N, ts=ts)
    live = unpack(m.mask, N)
    assert int(live.sum()) == m.live
    return live


@pytest.mark.parametrize("mode", ["u", "device_rng"])
def test_graphed_masked_span_step_is_the_eager_step(dev, oracle, synthetic, mode):
    from nerf_simple_amd import _lib as L
    from nerf_simple_amd import training as T
    from nerf_simple_amd.optim import FusedAdam
    B, N, seed, rid = 576, 64, 40, 3
    rays, gt, _ = (x.to(dev) for x in step_inputs(oracle, synthetic, B, N))
    us = [torch.rand(B, N, generator=torch.Generator().manual_seed(200 + k)).to(dev) for k in range(3)]
    occ, s = ball_grid(dev, "empty"), ball_span(dev)
    rng = mode == "device_rng"
    # three replays at a capacity that holds every step's live samples
    net, twin = make_net(dev, "structured"), make_net(dev, "structured")
    stepper = T.GraphedMaskedBoxTrainStep(net, FusedAdam(net, lr=0.0), B, N, s, occ, 1.0, device_rng=rng, seed=seed, ray_id0=rid)
    opt_twin = torch.optim.SGD(twin.parameters(), lr=0.0)
    for k in (1, 2, 3):
        ekw = dict(device_rng=True, seed=seed + k, ray_id0=rid) if rng else dict(u=us[k - 1])
        loss = stepper.step(rays, gt, u=None if rng else us[k - 1]).clone()
        want = T.train_step(twin, opt_twin, rays, gt, N, occupancy=occ, box=s, **ekw)
        assert same(loss, want), (mode, k, float(loss), float(want))
        assert stepper.counts()["live"] == occ.last_stats["live"] and same(stepper.ts, s.positions(rays, N, **ekw)), (mode, k)
        if k == 1:
            compare_gradients(grads_of(net), grads_of(twin), (mode, k))
    # one step at capacity exactly P', and with surplus rows
    u = us[0]
    ekw = dict(device_rng=True, seed=seed + 1, ray_id0=rid) if rng else dict(u=u)
    ts = s.positions(rays, N, **ekw)
    live = live_of(dev, occ, rays, N, ts)
    OM.require_informative(live, N, "empty")
    total = int(live.sum())
    twin = make_net(dev, "structured")
    want = T.train_step(twin, torch.optim.SGD(twin.parameters(), lr=0.0), rays, gt, N, occupancy=occ, box=s, **ekw)
    assert occ.last_stats["live"] == total
    for C in (total, min(-(-(total + 1) // 256) * 256, B * N)):
        net = make_net(dev, "structured")
        stepper = T.GraphedMaskedBoxTrainStep(net, FusedAdam(net, lr=0.0), B, N, s, occ, C, device_rng=rng, seed=seed, ray_id0=rid)
        loss = stepper.step(rays, gt, u=None if rng else u).clone()
        assert stepper.counts() == {"step": 1, "samples": B * N, "live": total, "kept": total, "capacity": C}
        assert same(loss, want), (mode, C, float(loss), float(want))
        assert same(stepper.ts, ts)
        compare_gradients(grads_of(net), grads_of(twin), (mode, C))
    # an overflowing capacity: the eager composition on the placed positions under mask_C
    C = -(-total // 2)
    assert C not in set(OM.offsets(live).tolist())                                # the capacity cuts inside a ray
    kept = G.mask_C(live, C)
    ref = make_net(dev, "structured")
    m = occ.mark(rays, N, ts=ts, points=True)
    mask_c, offsets_c = to_dev_mask(kept, dev)
    raw, _ = T._FusedDense.apply(ref, None, None, None, 0, 0, 0, 1, m.points[:C].contiguous(), *[p for _, p in ref.named_parameters()])
    rgb = T._MaskedVolumeRender.apply(raw.reshape(-1, 4), (rays, ts, None, L.FLAG_TS_GIVEN, 0, 0, mask_c, offsets_c), B, N)[0]
    want_c = T.mse_loss(rgb, gt)
    want_c.backward()
    net = make_net(dev, "structured")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        stepper = T.GraphedMaskedBoxTrainStep(net, FusedAdam(net, lr=0.0), B, N, s, occ, C, device_rng=rng, seed=seed, ray_id0=rid)
        loss = stepper.step(rays, gt, u=None if rng else u).clone()
        assert stepper.counts() == {"step": 1, "samples": B * N, "live": total, "kept": C, "capacity": C}
    assert same(loss, want_c.detach()) and not same(loss, want), (mode, float(loss), float(want_c))
    compare_gradients(grads_of(net), grads_of(ref), (mode, "overflow"))


def test_graphed_trajectory_follows_the_grid(dev, oracle, synthetic):
    """6 replays on ONE TrainingOccupancyGrid(33^3) that serves the span and the mask, device_rng=True, against 6 eager masked
    steps with seed + k: losses bit-equal at every step; the grid is updated in place before replay 4 and both the placement
    and the mark follow it without a new capture (lr = 0).  Then a replaced ``words`` tensor makes ``step`` raise."""
    from nerf_simple_amd import training as T
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.utils import mesh
    from nerf_simple_amd.utils.box import GridSpan, SceneBox
    from nerf_simple_amd.utils.occupancy import TrainingOccupancyGrid
    B, N, seed, R = 576, 64, 40, (33, 33, 33)
    rays, gt, _ = (x.to(dev) for x in step_inputs(oracle, synthetic, B, N))
    occ = TrainingOccupancyGrid(R, OG.BOUNDS, outside="empty", device=dev)
    s = GridSpan(occ)
    assert s.probes == 64
    net, twin, net_d, twin_d = (make_net(dev, "structured") for _ in range(4))
    stepper = T.GraphedMaskedBoxTrainStep(net, FusedAdam(net, lr=0.0), B, N, s, occ, 1.0, device_rng=True, seed=seed, ray_id0=11,
                                          check_every=2)
    dense = T.GraphedBoxTrainStep(net_d, FusedAdam(net_d, lr=0.0), B, N, s, device_rng=True, seed=seed, ray_id0=11)
    opt_twin, opt_d = (torch.optim.SGD(t.parameters(), lr=0.0) for t in (twin, twin_d))
    losses, lives, spans = [], [], []
    for k in range(1, 7):
        if k == 4:
            sigma = mesh.density_grid(net, R, OG.BOUNDS).cpu().numpy()
            ptr = occ.words.data_ptr()
            occ.update(net, float(np.percentile(sigma, 90)), decay=0.5, dilate=1)
            assert occ.words.data_ptr() == ptr
        loss, loss_d = stepper.step(rays, gt).clone(), dense.step(rays, gt).clone()
        ekw = dict(device_rng=True, seed=seed + k, ray_id0=11, box=s)
        want = T.train_step(twin, opt_twin, rays, gt, N, occupancy=occ, **ekw)
        assert same(loss, want), (k, float(loss), float(want))
        assert same(loss_d, T.train_step(twin_d, opt_d, rays, gt, N, **ekw)), k
        losses.append(float(loss))
        lives.append(occ.last_stats["live"])
        assert stepper.counts()["live"] == lives[-1], k
        # while every cell is live the span is the grid's own box, bit for bit; behind the update it no longer is
        jkw = dict(device_rng=True, seed=seed + k, ray_id0=11)
        spans.append(same(stepper.ts, SceneBox.from_grid(occ).positions(rays, N, **jkw)))
        assert same(stepper.ts, s.positions(rays, N, **jkw)), k
    assert stepper.overflow_steps == 0 and len(set(losses)) == 6
    assert lives[3] < lives[2] and spans == [True, True, True, False, False, False], (lives, spans)    # the mask AND the placement
    # a replaced words tensor is refused by both steppers: its address is baked into the placement node
    occ.words = occ.words.clone()
    for st in (stepper, dense):
        with pytest.raises(RuntimeError, match="words tensor was replaced"):
            st.step(rays, gt)
    assert stepper.opt.step_count == 6 and dense.opt.step_count == 6


def test_graphed_span_steps_select_their_own_rays(dev, oracle, synthetic):
    """rays_from with device_rng=True selects as before: every replay equals the eager step on the oracle's batch for
    (seed, step), bit for bit."""
    from nerf_simple_amd import training as T
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.utils.dataload import RayGenerator
    rays_tab = OG.full_rays(oracle, synthetic)
    gt_tab = torch.rand(rays_tab.shape[0], 3, generator=torch.Generator().manual_seed(21))
    n, B, N, seed = rays_tab.shape[0], 576, 64, 11
    rg = RayGenerator.from_tables(rays_tab, gt_tab, device=dev)
    occ, s = ball_grid(dev, "empty"), ball_span(dev)
    net_d, net_m, twin_d, twin_m = (make_net(dev, "structured") for _ in range(4))
    dense = T.GraphedBoxTrainStep(net_d, FusedAdam(net_d, lr=0.0), B, N, s, device_rng=True, seed=seed, rays_from=rg)
    masked = T.GraphedMaskedBoxTrainStep(net_m, FusedAdam(net_m, lr=0.0), B, N, s, occ, 0.99, device_rng=True, seed=seed, rays_from=rg)
    opt_d, opt_m = (torch.optim.SGD(t.parameters(), lr=0.0) for t in (twin_d, twin_m))
    for step in (1, 2, 3):
        ld, lm = dense.step().clone(), masked.step().clone()
        want = torch.from_numpy(oracle.select_ids_counter(n, B, seed, step))
        assert torch.equal(dense.ray_ids.cpu(), want) and torch.equal(masked.ray_ids.cpu(), want), step
        rays, gt = rays_tab[want].to(dev), gt_tab[want].to(dev)
        kw = dict(device_rng=True, seed=seed + step, box=s)
        assert same(ld, T.train_step(twin_d, opt_d, rays, gt, N, **kw)), step
        assert same(lm, T.train_step(twin_m, opt_m, rays, gt, N, occupancy=occ, **kw)), step
        assert masked.counts()["live"] == occ.last_stats["live"] <= masked.capacity, step
