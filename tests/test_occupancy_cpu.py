"""The occupancy grid and the masked render without a GPU: the numpy model against itself and the oracle, and the
library's host side (exports, size queries, argument checking -- no entry point touches a device here)."""
import ctypes

import numpy as np
import pytest
import torch

import occupancy_model as M

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R129 = (129, 129, 129)


def view_points(oracle, synthetic, N, n_side=100):
    """the issue's camera: pose (4, 30, 45), n_side x n_side rays, t in [2, 6], torch.manual_seed(0) jitter"""
    pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, 30, 45))).float()
    rays = oracle.camera_rays(pose, [n_side, n_side, synthetic.focal_from_fov(n_side)])
    torch.manual_seed(0)
    u = torch.rand(rays.shape[0], N)
    ts = oracle.sample_ts(u)
    q, dn = oracle.query_points(rays, ts)
    return rays, u, ts, q.reshape(rays.shape[0], N, 6), dn


# ---- the model against itself ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [(9, 9, 9), (7, 11, 6), (5, 4, 36), (4, 5, 67)])
@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_dilation_rule_separable_equals_direct(R, dilate):
    rng = np.random.default_rng(R[0] * 100 + dilate)
    sigma = rng.normal(size=R).astype(np.float32) * 3
    sigma[rng.random(R) < 0.003] = np.nan
    sigma[rng.random(R) < 0.003] = np.inf
    sigma[rng.random(R) < 0.02] = -np.inf
    for level in (6.0, 9.0):
        a = M.cells_from_density(sigma, level, dilate)
        b = M.cells_from_density_direct(sigma, level, dilate)
        assert a.shape == tuple(r - 1 for r in R) and np.array_equal(a, b)
        assert a.any() and (dilate > 0 or not a.all())          # neither all dead nor, undilated, all live
    # a NaN corner makes its cells live whatever the level
    s = np.full(R, -1.0, np.float32)
    s[1, 1, 1] = np.nan
    c = M.cells_from_density(s, 1e30, 0)
    assert c.sum() == 8 and c[:2, :2, :2].all()


@pytest.mark.parametrize("R", [(37, 41, 29), (5, 4, 33), (3, 3, 34), (4, 2, 66), (2, 2, 2)])
def test_packing_round_trip_and_padding(R):
    rng = np.random.default_rng(R[2])
    cells = rng.random(tuple(r - 1 for r in R)) < 0.4
    words = M.pack_bits(cells)
    assert words.dtype == np.uint32 and words.shape == (M.grid_words(R),)
    assert np.array_equal(M.unpack_bits(words, R), cells)
    wz, cz = M.words_per_row(R), R[2] - 1
    # cell (i, j, k) is bit k & 31 of word (i Cy + j) Wz + (k >> 5)
    for (i, j, k) in [(0, 0, 0), (R[0] - 2, R[1] - 2, cz - 1), ((R[0] - 2) // 2, (R[1] - 2) // 2, cz // 2)]:
        assert (int(words[(i * (R[1] - 1) + j) * wz + (k >> 5)]) >> (k & 31)) & 1 == int(cells[i, j, k])
    # padding bits of every row's last word are zero
    if cz % 32:
        last = words.reshape(-1, wz)[:, -1]
        assert not (last >> np.uint32(cz % 32)).any()
    assert int(sum(bin(int(x)).count("1") for x in words)) == int(cells.sum())


def test_cell_formula_edges():
    lo, step, inv = M.grid_axes((5, 5, 5), BOUNDS)
    cells = np.zeros((4, 4, 4), bool)
    cells[0, 0, 0] = cells[3, 3, 3] = True
    pts = np.array([[-1.5, -1.5, -1.5], [-1.6, 0, 0], [1.4999, 1.4999, 1.4999], [1.5, 1.5, 1.5], [np.nan, 0, 0],
                    [0, 0, np.inf], [0, 0, 0]], np.float32)
    assert M.sample_live(pts, cells, lo, inv, "empty").tolist() == [True, False, True, False, False, False, False]
    assert M.sample_live(pts, cells, lo, inv, "live").tolist() == [True, True, True, True, True, True, False]
    live = np.array([[1, 0, 1], [0, 0, 0]], bool)
    assert M.mask_words(live).tolist() == [[5], [0]] and M.offsets(live).tolist() == [0, 2, 2]
    wide = np.zeros((1, 130), bool)
    wide[0, [0, 63, 64, 129]] = True
    assert M.mask_words(wide).tolist() == [[1 | (1 << 63), 1, 2]]


# the issue's table: ball radius -> (live cells, live samples under 'empty', rays with no live sample, fullest ray)
TABLE = {1.0: (0.155, 0.131, 0.59, 65), 0.75: (0.066, 0.055, 0.78, 49), 0.5: (0.019, 0.016, 0.90, 33)}


def test_ball_table_reproduced(oracle, synthetic):
    N = 128
    _, _, _, q, _ = view_points(oracle, synthetic, N)
    lo, _, inv = M.grid_axes(R129, BOUNDS)
    pts = q[..., :3].numpy()
    inside = M.sample_live(pts, np.ones((128, 128, 128), bool), lo, inv, "empty")
    assert abs(inside.mean() - 0.662) <= 0.002
    for radius, (cell_frac, frac, empty, fullest) in TABLE.items():
        cells = M.ball_cells(R129, BOUNDS, radius)
        assert abs(cells.mean() - cell_frac) <= 0.002
        live = M.sample_live(pts, cells, lo, inv, "empty")
        f, most, none = M.stats(live)
        assert abs(f - frac) <= 0.002 and abs(none - empty) <= 0.01 and most == fullest, (radius, f, most, none)
    cells = M.ball_cells(R129, BOUNDS, 1.0)
    live = M.sample_live(pts, cells, lo, inv, "live")
    f, most, none = M.stats(live)
    assert abs(f - 0.47) <= 0.002 and none == 0.0
    for outside in ("empty", "live"):
        M.require_informative(M.sample_live(pts, cells, lo, inv, outside), N, outside)


@pytest.mark.parametrize("N", [1, 3, 64, 65, 128, 192, 768])
def test_ball_inputs_are_informative_at_every_N(oracle, synthetic, N):
    _, _, _, q, _ = view_points(oracle, synthetic, N)
    lo, _, inv = M.grid_axes(R129, BOUNDS)
    cells = M.ball_cells(R129, BOUNDS, 1.0)
    for outside, (a, b) in (("empty", (0.131, 0.135)), ("live", (0.469, 0.471))):
        live = M.sample_live(q[..., :3].numpy(), cells, lo, inv, outside)
        frac, fullest, empty = M.require_informative(live, N, outside)
        assert a - 0.002 <= frac <= b + 0.002 and fullest >= N / 2
        if outside == "empty":
            assert 0.59 - 0.01 <= empty <= 0.86 + 0.01


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_dead_rows_contribute_exactly_nothing(oracle, synthetic, dtype):
    N = 64
    rays, u, ts, q, dn = view_points(oracle, synthetic, N, n_side=24)
    sd = synthetic.synthetic_state_dict(0, "structured")
    with torch.no_grad():
        raw = oracle.nerf_forward(sd, q.reshape(-1, 6)).reshape(rays.shape[0], N, 4)
    lo, _, inv = M.grid_axes(R129, BOUNDS)
    live = M.sample_live(q[..., :3].numpy(), M.ball_cells(R129, BOUNDS, 1.0), lo, inv, "empty")
    assert 0.02 < live.mean() < 0.6 and (live.sum(1) == 0).any()
    raw, ts, dn = raw.to(dtype), ts.to(dtype), dn.to(dtype)
    rgb, disp, alpha, acc, w = M.masked_composite(oracle, raw, ts, dn, live)
    dead = torch.from_numpy(~live)
    assert torch.isfinite(rgb).all() and torch.isfinite(acc).all()
    assert (alpha[dead] == 0).all() and (w[dead] == 0).all()
    # against a composite that never looks at a dead sample: the per-sample weights, and the ray sums accumulated in
    # sample order, differ by exactly 0.0
    rgb_l, depth_l, acc_l, alpha_l, w_l = M.live_only_composite(raw, ts, dn, live)
    assert float((alpha - alpha_l).abs().max()) == 0.0 and float((w - w_l).abs().max()) == 0.0
    rgb_s, depth_s, acc_s = M.sequential_sums(w, M.masked_raw(raw, live), ts)
    assert float((rgb_s - rgb_l).abs().max()) == 0.0 and float((depth_s - depth_l).abs().max()) == 0.0
    assert float((acc_s - acc_l).abs().max()) == 0.0
    # torch.sum's own order may differ from sample order by rounding only
    eps = torch.finfo(dtype).eps
    assert float((rgb - rgb_l).abs().max()) <= 64 * eps * max(1.0, float(rgb_l.abs().max()))
    assert float((acc - acc_l).abs().max()) <= 64 * eps
    # a ray with no live sample: rgb = acc = 0 and NaN disparity, as the reference gives for acc == 0
    none = torch.from_numpy(live.sum(1) == 0)
    assert (rgb[none] == 0).all() and (acc[none] == 0).all() and torch.isnan(disp[none]).all()
    some = ~none
    assert torch.isfinite(disp[some & (acc > 0)]).all()


# ---- the library without a GPU -----------------------------------------------------------------------------------------
NEW = ("nerf_amd_occupancy_grid_words", "nerf_amd_occupancy_from_density", "nerf_amd_occupancy_from_mask",
       "nerf_amd_occupancy_mask_words", "nerf_amd_occupancy_workspace_bytes", "nerf_amd_occupancy_mark",
       "nerf_amd_occupancy_points", "nerf_amd_volume_render_masked", "nerf_amd_volume_render_masked_pixels")
EINVAL, EUNSUP = -1, -2


@pytest.fixture(scope="module")
def lib():
    import os
    from nerf_simple_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_new_symbols_exported_and_abi_unchanged(lib):
    from nerf_simple_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert hasattr(raw, s) and s in _lib.EXPORTS, s
    assert lib.nerf_amd_abi_version() == 5
    assert _lib.FLAG_OUTSIDE_EMPTY == 16


def test_size_queries_equal_the_model(lib):
    for R in ((129, 129, 129), (37, 41, 29), (2, 2, 2), (5, 4, 33), (3, 3, 34), (65, 65, 65)):
        assert lib.nerf_amd_occupancy_grid_words(*R) == M.grid_words(R), R
    for bad in ((1, 5, 5), (5, 5, 1), (0, 0, 0), (5, -3, 5), ((1 << 24) + 1, 2, 2)):
        assert lib.nerf_amd_occupancy_grid_words(*bad) == EINVAL, bad
    for B, N in ((1, 1), (63, 3), (1000, 64), (1000, 65), (10000, 128), (7, 192), (5, 768), (0, 128)):
        assert lib.nerf_amd_occupancy_mask_words(B, N) == B * ((N + 63) // 64)
    assert lib.nerf_amd_occupancy_mask_words(-1, 64) == EINVAL and lib.nerf_amd_occupancy_mask_words(4, 0) == EINVAL
    assert lib.nerf_amd_occupancy_mask_words(4, 769) == EUNSUP
    for B in (0, 1, 2048, 2049, 640000):
        n = lib.nerf_amd_occupancy_workspace_bytes(B)
        assert n >= 4 * B and n % 256 == 0          # at least one int32 count per ray
    assert lib.nerf_amd_occupancy_workspace_bytes(-1) == EINVAL


def test_entry_points_refuse_bad_arguments_on_the_host(lib):
    """Every call below must return before anything is launched: the pointers are fake."""
    P = ctypes.c_void_p(0x1000)           # a non-null, 16-aligned address that is never dereferenced
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    R = (9, 9, 9)
    # bits from sigma
    fd = lib.nerf_amd_occupancy_from_density
    assert fd(None, *R, 0.0, 1, P, None) == EINVAL and fd(P, *R, 0.0, 1, None, None) == EINVAL
    assert fd(P, 1, 9, 9, 0.0, 1, P, None) == EINVAL and fd(P, *R, 0.0, -1, P, None) == EINVAL
    assert fd(P, *R, 0.0, 16, P, None) == EUNSUP
    fm = lib.nerf_amd_occupancy_from_mask
    assert fm(None, *R, P, None) == EINVAL and fm(P, *R, None, None) == EINVAL and fm(P, 9, 1, 9, P, None) == EINVAL
    # mark
    mk = lib.nerf_amd_occupancy_mark

    def mark(rays=P, u=P, tbins=P, flags=0, bits=P, R=R, lo=f3, inv=f3, mask=P, offs=P, live=P, ws=P, B=4, N=64):
        return mk(rays, u, tbins, flags, 0, 0, bits, *R, lo, inv, mask, offs, live, ws, B, N, None)
    for kw in (dict(rays=None), dict(u=None), dict(tbins=None), dict(bits=None), dict(lo=None), dict(inv=None), dict(mask=None),
               dict(offs=None), dict(ws=None), dict(B=-1), dict(N=0), dict(N=-5), dict(flags=32), dict(flags=8),
               dict(flags=4), dict(R=(1, 9, 9)), dict(R=(9, 9, 0)), dict(offs=ctypes.c_void_p(0x1004))):
        assert mark(**kw) == EINVAL, kw
    assert mark(N=769) == EUNSUP and mark(N=769, flags=16) == EUNSUP
    # compacted points
    pt = lib.nerf_amd_occupancy_points

    def points(rays=P, u=P, tbins=P, flags=0, mask=P, offs=P, pts=P, cap=10, B=4, N=64):
        return pt(rays, u, tbins, flags, 0, 0, mask, offs, pts, cap, B, N, None)
    for kw in (dict(rays=None), dict(u=None), dict(tbins=None), dict(mask=None), dict(offs=None), dict(pts=None), dict(cap=-1),
               dict(B=-1), dict(N=0), dict(flags=16), dict(flags=64)):
        assert points(**kw) == EINVAL, kw
    assert points(N=769) == EUNSUP and points(B=0) == 0
    # masked composite, both output forms
    vr, vp = lib.nerf_amd_volume_render_masked, lib.nerf_amd_volume_render_masked_pixels

    def render(raw=P, rays=P, u=P, tbins=P, flags=0, mask=P, offs=P, rgb=P, disp=P, acc=P, B=4, N=64):
        return vr(raw, rays, u, tbins, flags, 0, 0, mask, offs, rgb, disp, None, acc, None, B, N, None)

    def pixels(raw=P, rays=P, u=P, tbins=P, flags=0, mask=P, offs=P, px=P, B=4, N=64):
        return vp(raw, rays, u, tbins, flags, 0, 0, mask, offs, px, B, N, None)
    for kw in (dict(rays=None), dict(u=None), dict(tbins=None), dict(mask=None), dict(offs=None), dict(B=-1), dict(N=0),
               dict(flags=16), dict(flags=128)):
        assert render(**kw) == EINVAL and pixels(**kw) == EINVAL, kw
    for kw in (dict(rgb=None), dict(disp=None), dict(acc=None)):
        assert render(**kw) == EINVAL, kw
    assert pixels(px=None) == EINVAL
    assert render(N=769) == EUNSUP and pixels(N=769) == EUNSUP
    assert render(B=0) == 0 and pixels(B=0) == 0


def test_cpu_tensors_raise_the_usual_error():
    from nerf_simple_amd.utils import nets, occupancy, rendering
    with pytest.raises(RuntimeError, match="GPU"):
        occupancy.OccupancyGrid.from_mask(torch.ones(4, 4, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="GPU"):
        occupancy.OccupancyGrid.from_density(torch.zeros(5, 5, 5), 0.0)
    net = nets.Nerf()
    with pytest.raises(TypeError, match="level"):
        occupancy.occupancy_grid(net, 16)
    with pytest.raises(RuntimeError):
        occupancy.occupancy_grid(net, 16, level=1.0)            # a CPU module: no CPU path
    # a render on CPU rays raises before the grid is looked at, and leaves torch's generator alone
    state = torch.get_rng_state()
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        rendering.render_nerf(torch.zeros(2, 6), net, 8, occupancy=object())
    assert torch.equal(torch.get_rng_state(), state)
