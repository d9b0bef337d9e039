"""The occupancy grid and the masked render on the GPU (csrc/occupancy.hip, utils/occupancy.py).

Masks, offsets and bits must equal the numpy restatement tests/occupancy_model.py exactly; the compacted points must be
rows of nerf_amd_query_points; the masked render must equal, bit for bit, the composition of entry points that existed before
it: nerf_amd_query_points -> nerf_amd_mlp_forward on all B N points -> dead rows overwritten with (0, 0, 0, -inf) ->
nerf_amd_volume_render_rays / _pixels.

Inputs: camera spherical_to_pose(4, 30, 45), 100 x 100 rays, t in [2, 6], torch.manual_seed(0) jitter, a 129^3 grid over
[-1.5, 1.5]^3 whose live cells are a ball of radius 1 judged at the cell centre.  Smaller ray sets are strided subsets.
"""
import warnings

import numpy as np
import pytest
import torch

import occupancy_model as M

pytestmark = pytest.mark.gpu

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R129 = (129, 129, 129)
BS = (1, 63, 1000, 10000)
NS = (1, 3, 64, 65, 128, 192, 768)
POLICIES = ("empty", "live")
NAMES = ("rgb", "disp", "alpha", "acc", "w")


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


def make_net(dev, kind, precision=None, sd=None):
    from nerf_simple_amd.utils import synthetic
    from nerf_simple_amd.utils.nets import Nerf
    net = Nerf(precision=precision).to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, kind) if sd is None else sd)
    return net


_scene = {}


def full_rays(oracle, synthetic):
    if "rays" not in _scene:
        pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, 30, 45))).float()
        _scene["pose"] = pose
        _scene["rays"] = oracle.camera_rays(pose, [100, 100, synthetic.focal_from_fov(100)]).contiguous()
    return _scene["rays"]


def full_u(N):
    if ("u", N) not in _scene:
        torch.manual_seed(0)
        _scene[("u", N)] = torch.rand(10000, N)
    return _scene[("u", N)]


def subset(B):
    if B == 10000:
        return np.arange(10000)
    return np.array([5050]) if B == 1 else np.linspace(0, 9999, B).astype(np.int64)


def ball():
    if "ball" not in _scene:
        _scene["ball"] = M.ball_cells(R129, BOUNDS, 1.0)
    return _scene["ball"]


def ball_grid(dev, outside):
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    key = ("grid", outside)
    if key not in _scene:
        _scene[key] = OccupancyGrid.from_mask(torch.from_numpy(ball()).to(dev), BOUNDS, outside=outside)
    return _scene[key]


def query_points(dev, rays, jit, tbins, flags, seed, ray_id0, N):
    from nerf_simple_amd.utils.rendering import _query_points
    return _query_points(rays, jit, tbins, flags, seed, ray_id0, N)


def tbins(N, dev):
    from nerf_simple_amd.utils.rendering import _tbins
    return _tbins(2, 6, N, dev)


def model_live(q, B, N, outside, key=None):
    """the model's live mask of query points q [B * N, 6]; `key` caches it for inputs that recur across tests"""
    if key is not None and ("live", key, B, N, outside) in _scene:
        return _scene[("live", key, B, N, outside)]
    lo, _, inv = M.grid_axes(R129, BOUNDS)
    live = M.sample_live(q.view(B, N, 6)[..., :3].cpu().numpy(), ball(), lo, inv, outside)
    if key is not None:
        _scene[("live", key, B, N, outside)] = live
    return live


def check_full_set_is_informative(dev, oracle, synthetic, N, outside):
    """the model's numbers for the full 10,000 rays, before anything is asked of the masked path"""
    key = ("info", N, outside)
    if key not in _scene:
        rays = full_rays(oracle, synthetic).to(dev)
        q, _ = query_points(dev, rays, full_u(N).to(dev), tbins(N, dev), 0, 0, 0, N)
        _scene[key] = M.require_informative(model_live(q, 10000, N, outside), N, outside)
    return _scene[key]


def composed(dev, net, code, rays, jit, tb, flags, seed, ray_id0, N, live, pixels=False):
    """the masked render out of entry points that existed before it (module docstring)"""
    from nerf_simple_amd import _lib
    lib = _lib.lib()
    B = rays.shape[0]
    q, ts = query_points(dev, rays, jit, tb, flags, seed, ray_id0, N)
    raw = torch.empty((B * N, 4), dtype=torch.float32, device=dev)
    st = _lib.stream_ptr(dev)
    _lib.check(lib.nerf_amd_mlp_forward(_lib.ptr(q), _lib.ptr(net.packed_weights(code)), _lib.ptr(raw), B * N, code, st), "forward")
    dead = torch.from_numpy(~np.asarray(live).reshape(-1)).to(dev)
    raw[dead] = torch.tensor([0.0, 0.0, 0.0, -np.inf], device=dev)
    if pixels:
        px = torch.empty((B, 4), dtype=torch.float32, device=dev)
        _lib.check(lib.nerf_amd_volume_render_pixels(_lib.ptr(raw), _lib.ptr(ts), _lib.ptr(rays), _lib.ptr(px), B, N, st), "pixels")
        return px
    outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in ((B, 3), (B,), (B, N), (B,), (B, N))]
    _lib.check(lib.nerf_amd_volume_render_rays(_lib.ptr(raw), _lib.ptr(ts), _lib.ptr(rays), *[_lib.ptr(o) for o in outs], B, N, st),
               "composite")
    if N == 1:
        outs[2], outs[4] = outs[2][:, :0], outs[4][:, :0]
    return tuple(outs)


# ---- 1. bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [(33, 33, 33), (37, 41, 29), (9, 7, 70), (5, 6, 34), (2, 2, 2)])
def test_bits_equal_the_model(dev, R):
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    rng = np.random.default_rng(R[0])
    sigma = (rng.normal(size=R) * 3).astype(np.float32)
    sigma[rng.random(R) < 0.004] = np.nan
    sigma[rng.random(R) < 0.004] = np.inf
    sigma[rng.random(R) < 0.02] = -np.inf
    vol = torch.from_numpy(sigma).to(dev)
    for dilate in (0, 1, 2):
        for level in (6.0, 9.0, -np.inf, np.inf):
            occ = OccupancyGrid.from_density(vol, level, BOUNDS, dilate)
            cells = M.cells_from_density(sigma, level, dilate)
            words = occ.words.cpu().numpy().view(np.uint32)
            assert np.array_equal(words, M.pack_bits(cells)), (R, dilate, level)
            assert np.array_equal(occ.cells().cpu().numpy(), cells)
            assert abs(occ.cell_fraction - cells.mean()) < 1e-12
    # a caller's own mask
    cells = rng.random(tuple(r - 1 for r in R)) < 0.3
    occ = OccupancyGrid.from_mask(torch.from_numpy(cells).to(dev), BOUNDS, outside="empty")
    assert np.array_equal(occ.words.cpu().numpy().view(np.uint32), M.pack_bits(cells))
    assert occ.resolution == R and occ.outside == "empty"


def test_occupancy_grid_of_a_network(dev):
    from nerf_simple_amd.utils import mesh
    from nerf_simple_amd.utils.occupancy import OccupancyGrid, occupancy_grid
    net = make_net(dev, "structured", "fp16")
    sigma = mesh.density_grid(net, 65, BOUNDS)
    level = float(sigma.median())
    a = occupancy_grid(net, 65, level, BOUNDS)
    b = OccupancyGrid.from_density(sigma, level, BOUNDS)
    assert torch.equal(a.words, b.words) and a.cell_fraction == b.cell_fraction
    assert np.array_equal(a.words.cpu().numpy().view(np.uint32), M.pack_bits(M.cells_from_density(sigma.cpu().numpy(), level, 1)))
    assert 0 < a.cell_fraction < 1
    with pytest.raises(TypeError):
        occupancy_grid(net, 65)


# ---- 2. mask, offsets, points -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["u", "ts", "device_rng"])
def test_mask_offsets_and_points_equal_the_model(dev, oracle, synthetic, mode):
    from nerf_simple_amd import _lib
    rays_all = full_rays(oracle, synthetic).to(dev)
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
                _, ts = query_points(dev, rays, u, tb, 0, 0, 0, N)
                kw, args = dict(ts=ts), (ts, None, _lib.FLAG_TS_GIVEN, 0, 0)
            else:
                kw, args = dict(device_rng=True, seed=7, ray_id0=12345), (None, tb, _lib.FLAG_DEVICE_RNG, 7, 12345)
            q, ts_k = query_points(dev, rays, *args, N)
            if mode != "device_rng":
                # torch's own o + d * t (two separately rounded operations) are the same points
                p = rays[:, None, :3] + rays[:, None, 3:] * ts_k[:, :, None]
                assert same(p.reshape(-1, 3), q[:, :3])
            for outside in POLICIES:
                live = model_live(q, B, N, outside)
                m = ball_grid(dev, outside).mark(rays, N, points=True, **kw)
                where = (mode, N, B, outside)
                assert np.array_equal(m.mask.cpu().numpy().view(np.uint64), M.mask_words(live)), where
                assert np.array_equal(m.offsets.cpu().numpy(), M.offsets(live)), where
                assert m.live == int(live.sum()) and m.points.shape == (m.live, 6), where
                assert same(m.points, q[torch.from_numpy(live.reshape(-1)).to(dev)]), where


# ---- 3. the render, bit for bit against the points-mode composition ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_masked_render_equals_the_composition_bit_for_bit(dev, oracle, synthetic, precision, kind):
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils.rendering import render_nerf
    net = make_net(dev, kind, precision)
    code = _lib.precision_code(precision)
    rays_all = full_rays(oracle, synthetic).to(dev)
    evaluated = 0
    for N in NS:
        for outside in POLICIES:
            check_full_set_is_informative(dev, oracle, synthetic, N, outside)
        for B in BS:
            idx = torch.from_numpy(subset(B)).to(dev)
            rays = rays_all[idx].contiguous()
            u = full_u(N).to(dev)[idx].contiguous()
            tb = tbins(N, dev)
            q, _ = query_points(dev, rays, u, tb, 0, 0, 0, N)
            for outside in POLICIES:
                live = model_live(q, B, N, outside, key="u")
                occ = ball_grid(dev, outside)
                want = composed(dev, net, code, rays, u, tb, 0, 0, 0, N, live)
                with torch.no_grad():
                    got = render_nerf(rays, net, N, u=u, occupancy=occ)
                for name, g, w in zip(NAMES, got, want):
                    assert same(g, w), (name, precision, kind, N, B, outside)
                assert occ.last_stats["live"] == int(live.sum()) and occ.last_stats["samples"] == B * N
                assert occ.last_stats["network_launches"] == (1 if live.any() else 0)
                evaluated += int(live.sum())
                # the pixel form, through the C ABI
                m = occ.mark(rays, N, u=u, points=True)
                px = torch.empty((B, 4), dtype=torch.float32, device=dev)
                raw = torch.empty((max(m.live, 1), 4), dtype=torch.float32, device=dev)
                lib, st = _lib.lib(), _lib.stream_ptr(dev)
                if m.live:
                    _lib.check(lib.nerf_amd_mlp_forward(_lib.ptr(m.points), _lib.ptr(net.packed_weights(code)), _lib.ptr(raw),
                                                        m.live, code, st), "forward")
                _lib.check(lib.nerf_amd_volume_render_masked_pixels(
                    _lib.ptr(raw), _lib.ptr(rays), _lib.ptr(u), _lib.ptr(tb), 0, 0, 0, _lib.ptr(m.mask), _lib.ptr(m.offsets),
                    _lib.ptr(px), B, N, st), "masked pixels")
                assert same(px, composed(dev, net, code, rays, u, tb, 0, 0, 0, N, live, pixels=True)), (precision, kind, N, B)
                if outside == "empty" and N >= 3 and B >= 1000:
                    assert torch.isfinite(got[0]).all() and (got[3] == 0).any() and (got[3] > 0).any()
    assert evaluated > 0
    from nerf_simple_amd.utils.nets import packed_status
    if code != _lib.F32:
        assert packed_status(net.packed_weights(code), code) == 0


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_render_view_through_the_grid(dev, oracle, synthetic, precision):
    from nerf_simple_amd.utils.rendering import generate_rays, render_nerf, render_view
    net = make_net(dev, "structured", precision)
    full_rays(oracle, synthetic)
    pose, cam = _scene["pose"].numpy(), [100, 100, synthetic.focal_from_fov(100)]
    N = 64
    for outside in POLICIES:
        occ = ball_grid(dev, outside)
        for ray0, n in ((0, 10000), (3777, 2500)):
            rays = generate_rays(pose, cam, dev, ray0, n)
            u = full_u(N).to(dev)[ray0:ray0 + n].contiguous()
            with torch.no_grad():
                for kw in (dict(device_rng=True, seed=11), dict(u=u)):
                    px = render_view(net, pose, cam, N=N, ray0=ray0, n_rays=n, precision=precision, occupancy=occ, **kw)
                    live = occ.last_stats["live"]
                    rgb, disp, _, acc, _ = render_nerf(rays, net, N, precision=precision, ray_id0=ray0, occupancy=occ,
                                                       outputs=("rgb", "disp", "acc"), **kw)
                    assert occ.last_stats["live"] == live and 0 < live < n * N
                    assert same(px, torch.cat([rgb.clamp(0., 1.), disp[:, None]], 1)), (precision, outside, ray0)


# ---- 4. all-live and all-dead grids ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_all_live_grid_is_the_dense_render_and_all_dead_is_nothing(dev, oracle, synthetic, precision):
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    from nerf_simple_amd.utils.rendering import render_nerf
    rays_all = full_rays(oracle, synthetic).to(dev)
    ones = torch.ones((128, 128, 128), dtype=torch.bool, device=dev)
    all_live = OccupancyGrid.from_mask(ones, BOUNDS, outside="live")
    all_dead = OccupancyGrid.from_mask(~ones, BOUNDS, outside="empty")
    assert all_live.cell_fraction == 1.0 and all_dead.cell_fraction == 0.0
    for kind in ("default", "structured"):
        net = make_net(dev, kind, precision)
        for B, N in ((1000, 128), (63, 65), (10000, 64), (1000, 768), (63, 1)):
            idx = torch.from_numpy(subset(B)).to(dev)
            rays, u = rays_all[idx].contiguous(), full_u(N).to(dev)[idx].contiguous()
            with torch.no_grad():
                for kw in (dict(u=u), dict(device_rng=True, seed=3, ray_id0=77)):
                    dense = render_nerf(rays, net, N, **kw)
                    got = render_nerf(rays, net, N, occupancy=all_live, **kw)
                    assert all_live.last_stats["live"] == B * N
                    for name, g, w in zip(NAMES, got, dense):
                        assert same(g, w), (name, precision, kind, B, N, sorted(kw))
                rgb, disp, alpha, acc, w = render_nerf(rays, net, N, u=u, occupancy=all_dead)
            assert all_dead.last_stats == {"rays": B, "samples": B * N, "live": 0, "network_launches": 0}
            assert (rgb == 0).all() and (acc == 0).all() and torch.isnan(disp).all()
            assert (alpha == 0).all() and (w == 0).all() and alpha.shape == ((B, N) if N > 1 else (B, 0))


# ---- 5. against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_masked_render_within_the_error_model(dev, oracle, synthetic, precision, kind):
    import error_model as E
    from nerf_simple_amd.utils.rendering import render_nerf
    N, B, outside = 128, 1000, "empty"
    check_full_set_is_informative(dev, oracle, synthetic, N, outside)
    idx = subset(B)
    rays, u = full_rays(oracle, synthetic)[idx].contiguous(), full_u(N)[idx].contiguous()
    sd = synthetic.synthetic_state_dict(0, kind)
    lo, _, inv = M.grid_axes(R129, BOUNDS)
    with torch.no_grad():
        ts = oracle.sample_ts(u)
        q, dn = oracle.query_points(rays, ts)
        live = M.sample_live(q.reshape(B, N, 6)[..., :3].numpy(), ball(), lo, inv, outside)
        assert 0.02 < live.mean() < 0.6
        want = M.masked_composite(oracle, oracle.nerf_forward(sd, q).reshape(B, N, 4), ts, dn, live)
        raw64 = oracle.nerf_forward({k: p.double() for k, p in sd.items()}, q.double()).reshape(B, N, 4)
        truth = M.masked_composite(oracle, raw64, ts.double(), dn.double(), live)
        want = {n: o.numpy() for n, o in zip(NAMES, want)}
        truth = {n: o.numpy() for n, o in zip(NAMES, truth)}
        bound32 = {n: E.FACTOR_32 * E.scaled_err(want[n], truth[n]) + E.ULP_FLOOR for n in NAMES}
        if precision == "fp32":
            bound, ref = bound32, truth
        else:
            emu = M.masked_composite(oracle, E.emulated_forward(sd, q, precision).reshape(B, N, 4), ts, dn, live)
            emu = {n: o.numpy() for n, o in zip(NAMES, emu)}
            bound, ref = {n: E.FACTOR_16 * E.scaled_err(emu[n], want[n]) + bound32[n] for n in NAMES}, want
        net = make_net(dev, kind, precision)
        got = render_nerf(rays.to(dev), net, N, u=u.to(dev), occupancy=ball_grid(dev, outside))
    got = {n: o.cpu().numpy() for n, o in zip(NAMES, got)}
    assert np.array_equal(np.isnan(got["disp"]), np.isnan(ref["disp"])) and np.isnan(got["disp"]).any()
    dead = ~live
    assert (got["alpha"][dead] == 0).all() and (got["w"][dead] == 0).all()
    for n in NAMES:
        err = E.scaled_err(got[n], ref[n])
        print(f"masked render {precision} {kind} {n}: scaled error {err:.3e}, bound {bound[n]:.3e}")
        assert np.isfinite(got[n][~np.isnan(ref[n])]).all()
        assert err <= bound[n], (n, precision, kind, err, bound[n])


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------
def test_two_calls_write_the_same_bytes(dev, oracle, synthetic):
    from nerf_simple_amd.utils.rendering import render_nerf
    net = make_net(dev, "structured", "fp16")
    rays = full_rays(oracle, synthetic).to(dev)
    N = 128
    occ = ball_grid(dev, "empty")
    runs = []
    for _ in range(2):
        m = occ.mark(rays, N, device_rng=True, seed=5, points=True)
        with torch.no_grad():
            out = render_nerf(rays, net, N, device_rng=True, seed=5, occupancy=occ)
        runs.append((m.mask, m.offsets, m.points) + tuple(out))
    assert 0 < runs[0][2].shape[0] < 10000 * N
    for a, b in zip(*runs):
        assert same(a, b)


# ---- 7. edges ------------------------------------------------------------------------------------------------------------------
def test_rays_that_miss_the_bounds_and_a_nan_origin(dev, oracle, synthetic):
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils.rendering import render_nerf
    net = make_net(dev, "structured", "fp32")
    N = 64
    # rays that leave the scene: every sample has z in [6, 10]
    away = torch.tensor([[0.1 * i, 0.0, 4.0, 0.0, 0.01 * i, 1.0] for i in range(8)], device=dev)
    u = full_u(N).to(dev)[:8].contiguous()
    tb = tbins(N, dev)
    for outside in POLICIES:
        occ = ball_grid(dev, outside)
        with torch.no_grad():
            got = render_nerf(away, net, N, u=u, occupancy=occ)
        q, _ = query_points(dev, away, u, tb, 0, 0, 0, N)
        live = model_live(q, 8, N, outside)
        assert live.all() if outside == "live" else not live.any()
        for name, g, w in zip(NAMES, got, composed(dev, net, _lib.F32, away, u, tb, 0, 0, 0, N, live)):
            assert same(g, w), (name, outside)
        if outside == "empty":
            assert (got[0] == 0).all() and (got[3] == 0).all() and torch.isnan(got[1]).all() and occ.last_stats["live"] == 0
        else:
            with torch.no_grad():
                for g, w in zip(got, render_nerf(away, net, N, u=u)):
                    assert same(g, w)
    # a NaN origin is outside the grid: it follows the policy, and under 'live' poisons its own ray only
    rays = full_rays(oracle, synthetic).to(dev)[torch.from_numpy(subset(63)).to(dev)].contiguous()
    rays[31, 0] = float("nan")
    u = full_u(N).to(dev)[:63].contiguous()
    q, _ = query_points(dev, rays, u, tb, 0, 0, 0, N)
    for outside in POLICIES:
        occ = ball_grid(dev, outside)
        live = model_live(q, 63, N, outside)
        assert live[31].all() if outside == "live" else not live[31].any()
        m = occ.mark(rays, N, u=u)
        assert np.array_equal(m.mask.cpu().numpy().view(np.uint64), M.mask_words(live))
        with torch.no_grad():
            got = render_nerf(rays, net, N, u=u, occupancy=occ)
        for name, g, w in zip(NAMES, got, composed(dev, net, _lib.F32, rays, u, tb, 0, 0, 0, N, live)):
            assert same(g, w), (name, outside)
        others = torch.arange(63, device=dev) != 31
        assert torch.isfinite(got[0][others]).all() and torch.isfinite(got[4][others]).all()
        if outside == "live":
            assert torch.isnan(got[0][31]).all() and torch.isnan(got[3][31])
        else:
            assert (got[0][31] == 0).all() and got[3][31] == 0 and torch.isnan(got[1][31])


def test_inference_only_and_unsupported_nets(dev, oracle, synthetic):
    from nerf_simple_amd.utils.nets import Nerf
    from nerf_simple_amd.utils.rendering import render_nerf, render_view
    occ = ball_grid(dev, "empty")
    rays = full_rays(oracle, synthetic).to(dev)[:16].contiguous()
    net = make_net(dev, "structured", "bf16")
    other_size = Nerf(6, 4, 256).to(dev)              # (nn.Linear's initialisers draw from the CPU generator: build it first)
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="inference only.*torch.no_grad"):
        render_nerf(rays, net, 16, occupancy=occ)                                   # a trainable net, grad enabled
    with pytest.raises(RuntimeError, match="inference only"):
        render_view(net, _scene["pose"].numpy(), [8, 8, synthetic.focal_from_fov(8)], N=16, occupancy=occ)
    for p in net.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="inference only"):
        render_nerf(rays.clone().requires_grad_(True), net, 16, occupancy=occ)      # rays that require grad
    render_nerf(rays, net, 16, device_rng=True, occupancy=occ)                      # frozen net, plain rays: fine
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="default Nerf"):
            render_nerf(rays, other_size, 16, occupancy=occ)

        class Foreign:
            def forward(self, q):
                return torch.zeros(q.shape[0], 4, device=q.device)
        with pytest.raises(RuntimeError, match="foreign nets"):
            render_nerf(rays, Foreign(), 16, occupancy=occ)
        with pytest.raises(RuntimeError, match="768"):
            render_nerf(rays, net, 769, device_rng=True, occupancy=occ)
        with pytest.raises(TypeError):
            render_nerf(rays, net, 16, occupancy="grid")
    assert torch.equal(torch.get_rng_state(), state), "a refused call must not consume the CPU generator"


def test_fp16_range_guard_through_the_masked_path(dev, oracle, synthetic):
    from nerf_simple_amd.utils.rendering import render_nerf
    sd = {k: v.clone() for k, v in synthetic.synthetic_state_dict(0, "structured").items()}
    gain = 1e5                               # function-preserving rescaling: the first hidden activations leave fp16's range
    sd["layers_0.0.weight"] *= gain
    sd["layers_0.0.bias"] *= gain
    sd["layers_0.2.weight"] /= gain
    net = make_net(dev, "structured", sd=sd)
    assert net.precision == "fp16"
    occ = ball_grid(dev, "empty")
    rays = full_rays(oracle, synthetic).to(dev)[torch.from_numpy(subset(1000)).to(dev)].contiguous()
    N = 64
    u = full_u(N).to(dev)[:1000].contiguous()
    with torch.no_grad():
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            got = render_nerf(rays, net, N, u=u, occupancy=occ)
        hits = [w for w in rec if "fp16 MFMA operands left their range" in str(w.message)]
        assert len(hits) == 1, [str(w.message) for w in rec]
        assert occ.last_stats["network_launches"] == 2 and occ.last_stats["live"] > 0      # fp16, then the repeat in bf16
        bf = render_nerf(rays, net, N, u=u, precision="bf16", occupancy=occ)
    for name, g, w in zip(NAMES, got, bf):
        assert same(g, w), name
    assert torch.isfinite(got[0]).all() and (got[3] > 0).any()


def test_reference_stream_is_consumed_as_the_dense_call_consumes_it(dev, oracle, synthetic):
    from nerf_simple_amd.utils.rendering import render_nerf
    net = make_net(dev, "structured", "fp16")
    occ = ball_grid(dev, "live")
    rays = full_rays(oracle, synthetic).to(dev)[torch.from_numpy(subset(1000)).to(dev)].contiguous()
    N = 64
    with torch.no_grad():
        torch.manual_seed(5)
        render_nerf(rays, net, N)
        after_dense = torch.get_rng_state()
        torch.manual_seed(5)
        got = render_nerf(rays, net, N, occupancy=occ)
        after_masked = torch.get_rng_state()
        torch.manual_seed(5)
        u = torch.rand(1000, N)                          # the reference's one B x N draw
        after_draw = torch.get_rng_state()
        want = render_nerf(rays, net, N, u=u.to(dev), occupancy=occ)
        torch.manual_seed(5)
        m = occ.mark(rays, N)
        after_mark = torch.get_rng_state()
    assert torch.equal(after_masked, after_dense) and torch.equal(after_masked, after_draw) and torch.equal(after_mark, after_draw)
    for name, g, w in zip(NAMES, got, want):
        assert same(g, w), name
    assert m.live == occ.last_stats["live"]
