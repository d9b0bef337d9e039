"""The scene box on the GPU (csrc/ray_box.hip, utils/box.py, training.GraphedBoxTrainStep / GraphedMaskedBoxTrainStep; DESIGN.md
section 33).  Yardstick: tests/box_model.py -- the definition op for op in fp32 (the kernel must equal it BIT FOR BIT) and in
float64 (within the bound derived there), on the case table tests/test_box_cpu.py checks class by class.

Kernel level: every jitter mode against the model; the invariants; poisoned guards behind every output; two runs, the same
bytes.  Render level: ``box=`` is the ``ts=`` path on ``box.positions`` bit for bit, through every precision, the grid and ray
termination; ``render_view`` is device ray generation -> placement -> render -> clip.  Step level, lr = 0: the eager step is
the step on the placed positions, the two graphed steppers are the eager step with seed + k (losses bit for bit, gradients
within the dW products' run-to-run tolerance).  Shapes, rays, grids and helpers: tests/test_gpu_occupancy_graphed.py."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import box_model as M
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


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def launch(dev, rays, jit, flags, seed, rid, N, *, span=True, hit=True, lo=M.LO, hi=M.HI, tn=M.TN, tf=M.TF):
    """nerf_amd_box_positions itself on pre-poisoned buffers with a guard of PAD elements behind each -> (ts, span, hit) on the
    CPU; the guards must come back untouched."""
    from nerf_simple_amd import _lib as L
    from nerf_simple_amd.utils.rendering import _tbins
    B = rays.shape[0]
    ts = torch.full((B * N + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    sp = torch.full((2 * B + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    ht = torch.full((B + PAD,), -7, dtype=torch.int32, device=dev)
    tb = None if flags & L.FLAG_TS_GIVEN else _tbins(0, 1, N, dev)
    jp = L.ptr(jit) if (jit is None or torch.is_tensor(jit)) else jit
    rc = L.lib().nerf_amd_box_positions(L.ptr(rays), jp, L.ptr(tb), flags, seed, rid, f3(lo), f3(hi), tn, tf, L.ptr(ts),
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


def check_invariants(ts, span, hit):
    assert not torch.isnan(ts).any() and not torch.isnan(span).any()
    assert bool(((ts >= span[:, :1]) & (ts <= span[:, 1:])).all())
    assert bool((ts[:, 1:] >= ts[:, :-1]).all())
    miss = hit == 0
    assert bool(((hit == 0) | (hit == 1)).all()) and bool(miss.any()) and not bool(miss.all())
    assert bool((span[miss] == torch.tensor([M.TN, M.TF])).all())
    assert bool((span[~miss, 0] < span[~miss, 1]).all())


# ---- 1.-3. the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_kernel_is_the_model(dev, B, N):
    from nerf_simple_amd import _lib as L
    from nerf_simple_amd.utils.rendering import _query_points, _tbins
    rays, _ = M.case_table(B)
    rd = rays.to(dev)
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(1000 * B + N))
    c = M.unit_positions(u, N)
    want = M.positions(rays, M.LO, M.HI, M.TN, M.TF, c)
    # explicit u
    got = launch(dev, rd, u.to(dev), 0, 0, 0, N)
    assert same3(got, want), (B, N)
    check_invariants(*got)
    # given unit positions
    assert same3(launch(dev, rd, c.to(dev), L.FLAG_TS_GIVEN, 0, 0, N), want), (B, N)
    # the counter RNG: its unit positions are nerf_amd_query_points' on unit bins, same seed, same ray ids
    seed, rid, off = 77 + N, 5 * B, 3
    c_rng = _query_points(rd, None, _tbins(0, 1, N, dev), L.FLAG_DEVICE_RNG, seed, rid, N)[1].cpu()
    assert bool((c_rng >= 0).all()) and bool((c_rng <= 1).all()) and not same(c_rng, c)
    want_rng = M.positions(rays, M.LO, M.HI, M.TN, M.TF, c_rng)
    got_rng = launch(dev, rd, None, L.FLAG_DEVICE_RNG, seed, rid, N)
    assert same3(got_rng, want_rng), (B, N)
    check_invariants(*got_rng)
    assert not same(launch(dev, rd, None, L.FLAG_DEVICE_RNG, seed, rid + 1, N)[0], got_rng[0])       # the ray ids matter
    # the seed in memory: the bare seed plus the offset
    mem = torch.tensor([off], dtype=torch.int64, device=dev)
    got_mem = launch(dev, rd, ctypes.c_void_p(mem.data_ptr()), L.FLAG_DEVICE_RNG | L.FLAG_SEED_IN_MEMORY, seed - off, rid, N)
    assert same3(got_mem, got_rng), (B, N)
    # float64: within the derived bound wherever the two models agree about the hit; a disagreement is a grazing ray
    r64, c64 = rays.double(), M.unit_positions(u, N, torch.float64)
    ts64, _, hit64 = M.positions(r64, M.LO, M.HI, M.TN, M.TF, c64)
    assert M.agree_or_grazing(got[2], r64, M.LO, M.HI, M.TN, M.TF)
    agree = got[2] == hit64
    ratio = ((got[0].double() - ts64).abs() / M.bound(c64, M.TN, M.TF))[agree]
    print(f"box positions vs float64, B={B} N={N}: worst {float(ratio.max()):.3f} of the derived bound")
    assert float(ratio.max()) <= 1.0, (B, N, float(ratio.max()))
    # NULL span / hit are skipped, ts is what it was; two runs write the same bytes
    assert same(launch(dev, rd, u.to(dev), 0, 0, 0, N, span=False, hit=False)[0], got[0])
    assert same3(launch(dev, rd, u.to(dev), 0, 0, 0, N), got)


def test_empty_problem_and_python_call(dev):
    from nerf_simple_amd import _lib as L
    from nerf_simple_amd.utils.box import SceneBox
    one = torch.zeros(8, device=dev)
    assert L.lib().nerf_amd_box_positions(None, L.ptr(one), L.ptr(one), 0, 0, 0, f3(M.LO), f3(M.HI), 2.0, 6.0, None, None, None, 0, 64,
                                          L.stream_ptr(dev)) == 0
    B, N = 37, 65
    rays, _ = M.case_table(B)
    rd = rays.to(dev)
    b = SceneBox(M.LO, M.HI)
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(4))
    want = M.positions(rays, M.LO, M.HI, M.TN, M.TF, M.unit_positions(u, N))
    ts, span, hit = b.positions(rd, N, u=u.to(dev), return_span=True)
    assert same3((ts.cpu(), span.cpu(), hit.cpu()), want) and hit.dtype == torch.int32
    assert same(b.positions(rd, N, u=u.to(dev)), ts) and not ts.requires_grad
    assert same(b.positions(rd.clone().requires_grad_(True), N, u=u.to(dev)), ts)
    # the default jitter is the reference's one torch.rand(B, N), and leaves the generator where the reference leaves it
    torch.manual_seed(11)
    got = b.positions(rd, N)
    state = torch.get_rng_state()
    torch.manual_seed(11)
    u_ref = torch.rand(B, N)
    assert torch.equal(torch.get_rng_state(), state)
    assert same(got.cpu(), M.positions(rays, M.LO, M.HI, M.TN, M.TF, M.unit_positions(u_ref, N))[0])
    # a refused call leaves the generator where it was
    for call in (lambda: b.positions(rd, 769), lambda: b.positions(rd, N, tn=6, tf=2), lambda: b.positions(rd, N, u=u.to(dev)[:, :3]),
                 lambda: b.positions(rd[:, :5], N)):
        with pytest.raises((RuntimeError, ValueError)):
            call()
    assert torch.equal(torch.get_rng_state(), state)


# ---- 4. the renders ------------------------------------------------------------------------------------------------------------
def ball_box(dev):
    from nerf_simple_amd.utils.box import SceneBox
    return SceneBox.from_occupancy(ball_grid(dev, "empty"))


def test_box_of_the_ball_grid(dev):
    from nerf_simple_amd.utils.box import SceneBox
    occ = ball_grid(dev, "empty")
    b = ball_box(dev)
    step = 3.0 / 128
    for a in range(3):                                     # the radius-1 ball's cells, one cell of margin: a little beyond +-1
        assert -1.0 - 4 * step <= b.lo[a] <= -1.0 + step and 1.0 - step <= b.hi[a] <= 1.0 + 4 * step, b
    wide = SceneBox.from_occupancy(occ, margin=1000)
    assert wide == SceneBox.from_grid(occ) == SceneBox(*OG.BOUNDS)
    tight = SceneBox.from_occupancy(occ, margin=0)
    assert all(b.lo[a] < tight.lo[a] and tight.hi[a] < b.hi[a] for a in range(3))
    dead = type(occ).from_mask(torch.zeros(4, 4, 4, dtype=torch.bool, device=dev), OG.BOUNDS)
    with pytest.raises(ValueError, match="no live cell"):
        SceneBox.from_occupancy(dead)


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_render_nerf_box_is_its_ts_path(dev, oracle, synthetic, precision):
    from nerf_simple_amd.utils.occupancy import EarlyTermination
    from nerf_simple_amd.utils.rendering import render_nerf
    B, N = 576, 64
    rays, _, u = (x.to(dev) for x in step_inputs(oracle, synthetic, B, N))
    net = make_net(dev, "structured", precision)
    b = ball_box(dev)
    ts = b.positions(rays, N, u=u)
    with torch.no_grad():
        got, want = render_nerf(rays, net, N, box=b, u=u), render_nerf(rays, net, N, ts=ts)
        assert all(same(g, w) for g, w in zip(got, want)), precision
        assert not same(got[0], render_nerf(rays, net, N, u=u)[0])                                 # the box did matter
        kw = dict(device_rng=True, seed=9, ray_id0=100)
        got, want = render_nerf(rays, net, N, box=b, **kw), render_nerf(rays, net, N, ts=b.positions(rays, N, **kw))
        assert all(same(g, w) for g, w in zip(got, want)), precision
        for outside in OG.POLICIES:
            occ = ball_grid(dev, outside)
            got, want = render_nerf(rays, net, N, box=b, u=u, occupancy=occ), render_nerf(rays, net, N, ts=ts, occupancy=occ)
            assert all(same(g, w) for g, w in zip(got, want)), (precision, outside)
        term, occ = EarlyTermination(1e-3, 32), ball_grid(dev, "empty")
        for path in (dict(terminate=term), dict(terminate=term, occupancy=occ)):
            got, want = render_nerf(rays, net, N, box=b, u=u, **path), render_nerf(rays, net, N, ts=ts, **path)
            assert all(same(g, w) for g, w in zip(got, want)), (precision, sorted(path))
        # the default jitter: one reference draw, consumed as the reference consumes it
        torch.manual_seed(5)
        got = render_nerf(rays, net, N, box=b)
        state = torch.get_rng_state()
        torch.manual_seed(5)
        want = render_nerf(rays, net, N, ts=b.positions(rays, N, u=torch.rand(B, N).to(dev)))
        assert torch.equal(torch.get_rng_state(), state) and all(same(g, w) for g, w in zip(got, want))


def test_render_view_and_evaluate(dev, oracle, synthetic):
    from nerf_simple_amd.utils import metrics as MT
    from nerf_simple_amd.utils.dataload import RayGenerator
    from nerf_simple_amd.utils.rendering import generate_rays, render_nerf, render_view
    S, N = 24, 64
    cam = [S, S, synthetic.focal_from_fov(S)]
    pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, -30, 0))).float()
    net = make_net(dev, "structured", "fp16")
    b = ball_box(dev)
    u = torch.rand(S * S, N, generator=torch.Generator().manual_seed(2)).to(dev)
    rays = generate_rays(pose, cam, dev)

    def composed(ts, **kw):
        rgb, disp, _, _, _ = render_nerf(rays, net, N, ts=ts, **kw)
        return torch.cat([rgb.clamp(0., 1.), disp[:, None]], dim=1)

    with torch.no_grad():
        ts = b.positions(rays, N, u=u)
        assert same(render_view(net, pose, cam, N=N, u=u, box=b), composed(ts))
        assert not same(render_view(net, pose, cam, N=N, u=u, box=b), render_view(net, pose, cam, N=N, u=u))
        for outside in OG.POLICIES:
            occ = ball_grid(dev, outside)
            assert same(render_view(net, pose, cam, N=N, u=u, box=b, occupancy=occ), composed(ts, occupancy=occ)), outside
        bg = torch.tensor([0.25, 0.5, 0.75], device=dev)
        assert same(render_view(net, pose, cam, N=N, u=u, box=b, background=bg), composed(ts, background=bg))
        # the counter RNG is keyed by global pixel id: a pixel range is that range of the whole view
        whole = render_view(net, pose, cam, N=N, device_rng=True, seed=4, box=b)
        assert same(whole, composed(b.positions(rays, N, device_rng=True, seed=4)))
        assert same(render_view(net, pose, cam, N=N, device_rng=True, seed=4, box=b, ray0=100, n_rays=200), whole[100:300])
        with pytest.raises(RuntimeError, match="n_rays, N"):
            render_view(net, pose, cam, N=N, u=u[:, :5], box=b)
    # evaluate passes box= on to render_view
    gen = np.random.default_rng(5)
    samples = {"val": [{"img": gen.random((16, 16, 3), dtype=np.float32), "transform": oracle.spherical_to_pose(4, -30, 40.0 * i)}
                       for i in range(2)]}
    cam16 = [16, 16, synthetic.focal_from_fov(16)]
    rg = RayGenerator.from_samples(samples, cam16, dev)
    out = MT.evaluate(net, rg, "val", N=16, device_rng=True, box=b)
    by_hand = MT.evaluate(net, rg, "val", render=lambda p: render_view(net, p, cam16, N=16, device_rng=True, box=b))
    assert out == by_hand and out["views"] == 2 and out != MT.evaluate(net, rg, "val", N=16, device_rng=True)


# ---- 5. what the box buys --------------------------------------------------------------------------------------------------------
def unpack(mask, N):
    """mask words int64 [B, W] -> bool [B, N] (numpy)"""
    bit = (mask[:, :, None] >> torch.arange(64, device=mask.device)) & 1
    return bit.reshape(mask.shape[0], -1)[:, :N].bool().cpu().numpy()


@pytest.mark.parametrize("N", [64, 130])
def test_the_box_raises_the_live_count(dev, oracle, synthetic, N):
    rays = OG.full_rays(oracle, synthetic).to(dev)
    u = torch.rand(rays.shape[0], N, generator=torch.Generator().manual_seed(N)).to(dev)
    occ = ball_grid(dev, "empty")
    b = ball_box(dev)
    ts, span, hit = b.positions(rays, N, u=u, return_span=True)
    plain, boxed = occ.mark(rays, N, u=u), occ.mark(rays, N, ts=ts)
    for m in (plain, boxed):
        OM.require_informative(unpack(m.mask, N), N, "empty")
    per_ray = (boxed.offsets[1:] - boxed.offsets[:-1]).cpu()
    miss = hit.cpu() == 0
    print(f"N={N}: live {plain.live} -> {boxed.live} of {rays.shape[0] * N}; {int(miss.sum())} rays miss the box; "
          f"live per hit ray {boxed.live / max(1, int((~miss).sum())):.1f}")
    assert boxed.live > plain.live
    assert bool(miss.any()) and not bool(per_ray[miss].any())                    # a miss is dead as a whole behind this grid
    assert bool((span.cpu()[miss] == torch.tensor([2.0, 6.0])).all())


# ---- 6. the steps, lr = 0 --------------------------------------------------------------------------------------------------------
def grads_of(net):
    return {k: p.grad.clone() for k, p in net.named_parameters()}


def test_eager_step_is_the_step_on_the_placed_positions(dev, oracle, synthetic):
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils.rendering import render_nerf
    B, N = 576, 64
    rays, gt, u = (x.to(dev) for x in step_inputs(oracle, synthetic, B, N))
    b = ball_box(dev)
    ts = b.positions(rays, N, u=u)
    for occ in (None, ball_grid(dev, "empty")):
        net, twin = make_net(dev, "structured"), make_net(dev, "structured")
        okw = {} if occ is None else dict(occupancy=occ)
        loss = T.train_step(net, torch.optim.SGD(net.parameters(), lr=0.0), rays, gt, N, u=u, box=b, **okw)
        rgb = (render_nerf(rays, twin, N, ts=ts) if occ is None else T.render_nerf_masked(rays, twin, N, occ, ts=ts))[0]
        want = T.mse_loss(rgb, gt)
        assert same(loss, want.detach()), (occ is None, float(loss), float(want))
        want.backward()
        compare_gradients(grads_of(net), grads_of(twin), ("eager", occ is None))
        other = make_net(dev, "structured")
        plain = T.train_step(other, torch.optim.SGD(other.parameters(), lr=0.0), rays, gt, N, u=u, **okw)
        assert not same(loss, plain)
    # the exact fp32 path takes given positions, so it takes the box
    net, twin = make_net(dev, "structured", "fp32"), make_net(dev, "structured", "fp32")
    loss = T.train_step(net, torch.optim.SGD(net.parameters(), lr=0.0), rays[:64], gt[:64], N, u=u[:64], box=b, precision="fp32")
    want = T.mse_loss(render_nerf(rays[:64], twin, N, ts=ts[:64].contiguous(), precision="fp32")[0], gt[:64])
    assert same(loss, want.detach())
    # the three controls through the grid: the torch expression on the masked render of the placed positions; the distortion
    # term keeps the global tf
    occ = ball_grid(dev, "empty")
    bg = torch.rand(B, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    c = T.Controls(background=bg, sigma_noise=STD, noise_seed=41, distortion=LAM)
    net, twin = make_net(dev, "default"), make_net(dev, "default")
    loss = T.train_step(net, torch.optim.SGD(net.parameters(), lr=0.0), rays, gt, N, u=u, ray_id0=9, occupancy=occ, box=b, controls=c)
    rgb, _, _, acc, w = T.render_nerf_masked(rays, twin, N, occ, ts=ts, ray_id0=9, controls=T.Controls(sigma_noise=STD, noise_seed=41))
    assert same(w.ts, ts)
    term = T._distortion_term(w, w.ts, LAM, 2, 6)
    want = T.mse_loss(rgb + (1 - acc)[:, None] * bg, gt) + term
    assert same(loss, want.detach()) and same(loss.distortion, term.detach()) and float(term.detach()) > 0


@pytest.mark.parametrize("mode", ["u", "device_rng"])
def test_graphed_box_step_is_the_eager_step(dev, oracle, synthetic, mode):
    from nerf_simple_amd import training as T
    from nerf_simple_amd.optim import FusedAdam
    B, N, seed, rid = 576, 64, 40, 3
    rays, gt, _ = (x.to(dev) for x in step_inputs(oracle, synthetic, B, N))
    us = [torch.rand(B, N, generator=torch.Generator().manual_seed(100 + k)).to(dev) for k in range(3)]
    b = ball_box(dev)
    rng = mode == "device_rng"
    net, twin = make_net(dev, "structured"), make_net(dev, "structured")
    stepper = T.GraphedBoxTrainStep(net, FusedAdam(net, lr=0.0), B, N, b, device_rng=rng, seed=seed, ray_id0=rid, check_every=2)
    opt_twin = torch.optim.SGD(twin.parameters(), lr=0.0)
    seen = []
    for k in (1, 2, 3):
        ekw = dict(device_rng=True, seed=seed + k, ray_id0=rid) if rng else dict(u=us[k - 1])
        loss = stepper.step(rays, gt, u=None if rng else us[k - 1]).clone()
        want = T.train_step(twin, opt_twin, rays, gt, N, box=b, **ekw)
        assert same(loss, want), (mode, k, float(loss), float(want))
        assert same(stepper.ts_box, b.positions(rays, N, **ekw)) and same(stepper.ts, stepper.ts_box), (mode, k)
        if k == 1:
            compare_gradients(grads_of(net), grads_of(twin), (mode, k))
        seen.append(float(loss))
    assert len(set(seen)) == 3                                                    # the jitter moved with the step
    assert not same(loss, T.train_step(twin, opt_twin, rays, gt, N, **ekw))       # the box did matter
    # with every control on: the dense head behind the same placement
    bg = torch.rand(3, generator=torch.Generator().manual_seed(8)).to(dev)
    c = T.Controls(background=bg, sigma_noise=STD, noise_seed=900, distortion=LAM)
    net2 = make_net(dev, "structured")
    full = T.GraphedBoxTrainStep(net2, FusedAdam(net2, lr=0.0), B, N, b, device_rng=rng, seed=seed, ray_id0=rid, controls=c)
    for k in (1, 2):
        ekw = dict(device_rng=True, seed=seed + k) if rng else dict(u=us[k - 1])
        loss = full.step(rays, gt, u=None if rng else us[k - 1]).clone()
        want = T.train_step(twin, opt_twin, rays, gt, N, box=b, ray_id0=rid, controls=c.replace(noise_seed=c.noise_seed + k), **ekw)
        assert same(loss, want) and same(full.distortion, want.distortion) and float(want.distortion) > 0, (mode, k)


def live_of_box(dev, occ, rays, N, ts):
    m = occ.mark(rays, N, ts=ts)
    live = unpack(m.mask, N)
    assert int(live.sum()) == m.live
    return live


@pytest.mark.parametrize("mode", ["u", "device_rng"])
def test_graphed_masked_box_step_is_the_eager_step(dev, oracle, synthetic, mode):
    from nerf_simple_amd import training as T
    from nerf_simple_amd.optim import FusedAdam
    B, N, seed, rid = 576, 64, 40, 3
    rays, gt, u = (x.to(dev) for x in step_inputs(oracle, synthetic, B, N))
    occ, b = ball_grid(dev, "empty"), ball_box(dev)
    rng = mode == "device_rng"
    ekw = dict(device_rng=True, seed=seed + 1, ray_id0=rid) if rng else dict(u=u)
    ts = b.positions(rays, N, **ekw)
    live = live_of_box(dev, occ, rays, N, ts)
    OM.require_informative(live, N, "empty")
    total = int(live.sum())
    twin = make_net(dev, "structured")
    want = T.train_step(twin, torch.optim.SGD(twin.parameters(), lr=0.0), rays, gt, N, occupancy=occ, box=b, **ekw)
    assert occ.last_stats["live"] == total
    for C in (total, min(-(-(total + 1) // 256) * 256, B * N)):                   # exactly, and with surplus rows
        net = make_net(dev, "structured")
        stepper = T.GraphedMaskedBoxTrainStep(net, FusedAdam(net, lr=0.0), B, N, b, occ, C, device_rng=rng, seed=seed, ray_id0=rid)
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
    from nerf_simple_amd import _lib as L
    rgb = T._MaskedVolumeRender.apply(raw.reshape(-1, 4), (rays, ts, None, L.FLAG_TS_GIVEN, 0, 0, mask_c, offsets_c), B, N)[0]
    want_c = T.mse_loss(rgb, gt)
    want_c.backward()
    net = make_net(dev, "structured")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        stepper = T.GraphedMaskedBoxTrainStep(net, FusedAdam(net, lr=0.0), B, N, b, occ, C, device_rng=rng, seed=seed, ray_id0=rid)
        loss = stepper.step(rays, gt, u=None if rng else u).clone()
        assert stepper.counts() == {"step": 1, "samples": B * N, "live": total, "kept": C, "capacity": C}
    assert same(loss, want_c.detach()) and not same(loss, want), (mode, float(loss), float(want_c))
    compare_gradients(grads_of(net), grads_of(ref), (mode, "overflow"))


def test_graphed_masked_box_trajectory(dev, oracle, synthetic):
    """6 replays with all three controls and device_rng=True against 6 eager masked steps with seed + k and noise_seed + k,
    losses and distortion terms bit-equal at every step; the grid is updated in place behind replay 3 (lr = 0, as
    tests/test_gpu_masked_controls.py::test_graphed_trajectory_with_controls explains)."""
    from nerf_simple_amd import training as T
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.utils import mesh
    from nerf_simple_amd.utils.box import SceneBox
    from nerf_simple_amd.utils.occupancy import TrainingOccupancyGrid
    B, N, seed, R = 576, 64, 40, (33, 33, 33)
    rays, gt, _ = (x.to(dev) for x in step_inputs(oracle, synthetic, B, N))
    occ = TrainingOccupancyGrid(R, OG.BOUNDS, outside="empty", device=dev)
    b = SceneBox((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    bg = torch.rand(B, 3, generator=torch.Generator().manual_seed(8)).to(dev)
    c = T.Controls(background=bg, sigma_noise=STD, noise_seed=900, distortion=LAM)
    net, twin = make_net(dev, "structured"), make_net(dev, "structured")
    stepper = T.GraphedMaskedBoxTrainStep(net, FusedAdam(net, lr=0.0), B, N, b, occ, 1.0, device_rng=True, seed=seed, ray_id0=11,
                                          controls=c, check_every=2)
    opt_twin = torch.optim.SGD(twin.parameters(), lr=0.0)
    losses, lives = [], []
    for k in range(1, 7):
        if k == 4:
            sigma = mesh.density_grid(net, R, OG.BOUNDS).cpu().numpy()
            occ.update(net, float(np.percentile(sigma, 90)), decay=0.5, dilate=1)
        loss = stepper.step(rays, gt).clone()
        want = T.train_step(twin, opt_twin, rays, gt, N, device_rng=True, seed=seed + k, ray_id0=11, occupancy=occ, box=b,
                            controls=c.replace(noise_seed=c.noise_seed + k))
        assert same(loss, want), (k, float(loss), float(want))
        assert same(stepper.distortion, want.distortion), k
        losses.append(float(loss))
        lives.append(occ.last_stats["live"])
    assert stepper.counts()["live"] == lives[-1] and stepper.overflow_steps == 0
    assert lives[3] < lives[2] and len(set(losses)) == 6
    # the tight box of the updated grid is another stepper (the box is baked into the graph by value)
    tight = SceneBox.from_occupancy(occ)
    assert tight != b and stepper.box is b


def test_graphed_box_steps_select_their_own_rays(dev, oracle, synthetic):
    """rays_from with device_rng=True: the selection runs on graph A's side branch; the placement in front of the forward reads
    the batch it left.  Every replay equals the eager step on the oracle's batch for (seed, step), bit for bit."""
    from nerf_simple_amd import training as T
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.utils.dataload import RayGenerator
    rays_tab = OG.full_rays(oracle, synthetic)
    gt_tab = torch.rand(rays_tab.shape[0], 3, generator=torch.Generator().manual_seed(21))
    n, B, N, seed = rays_tab.shape[0], 576, 64, 11
    rg = RayGenerator.from_tables(rays_tab, gt_tab, device=dev)
    occ, b = ball_grid(dev, "empty"), ball_box(dev)
    net_d, net_m, twin_d, twin_m = (make_net(dev, "structured") for _ in range(4))
    dense = T.GraphedBoxTrainStep(net_d, FusedAdam(net_d, lr=0.0), B, N, b, device_rng=True, seed=seed, rays_from=rg)
    masked = T.GraphedMaskedBoxTrainStep(net_m, FusedAdam(net_m, lr=0.0), B, N, b, occ, 0.75, device_rng=True, seed=seed, rays_from=rg)
    opt_d, opt_m = (torch.optim.SGD(t.parameters(), lr=0.0) for t in (twin_d, twin_m))
    for step in (1, 2, 3):
        ld, lm = dense.step().clone(), masked.step().clone()
        want = torch.from_numpy(oracle.select_ids_counter(n, B, seed, step))
        assert torch.equal(dense.ray_ids.cpu(), want) and torch.equal(masked.ray_ids.cpu(), want), step
        rays, gt = rays_tab[want].to(dev), gt_tab[want].to(dev)
        kw = dict(device_rng=True, seed=seed + step, box=b)
        assert same(ld, T.train_step(twin_d, opt_d, rays, gt, N, **kw)), step
        assert same(lm, T.train_step(twin_m, opt_m, rays, gt, N, occupancy=occ, **kw)), step
        assert masked.counts()["live"] == occ.last_stats["live"] <= masked.capacity, step
