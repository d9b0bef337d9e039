"""nerf_amd_image_metrics and utils/metrics.py on the GPU, against the float64 definition of tests/ssim_model.py.

Bounds (none of them read off the GPU):
  * every map value, and every per-image ssim_c (the mean is formed in double), within (2 C_REF_SSIM + 4) 2^-24 of float64:
    the project's 2 c + 4 rule on the measured error of the fp32 yardstick (tests/test_metrics_cpu.py);
  * pred is gt: every map value and ssim exactly 1.0 -- numerator and denominator are the same fp32 numbers;
  * |sse - sse64| <= 4 2^-24 sse64: one rounding in the difference, doubled by the square, one in the product, a double sum;
  * max_gt bit-equal to gt[..., :3].max();  psnr_ref within what the sse bound implies, 10 / ln 10 of it.
Shapes: one window, thin images, and with T = 32 the tile edge: the last tile one position short, exact, one over; two tiles by
one; 70 x 45."""
import math

import numpy as np
import pytest
import torch

import ssim_model as SM

pytestmark = pytest.mark.gpu

DEV = "cuda"
T = SM.TILE
BOUND = (2 * SM.C_REF_SSIM + 4) * SM.EPS
SSE_REL = 4 * SM.EPS
SHAPES = [(11, 11), (11, 40), (40, 11), (12, 13), (T + 9, T + 9), (T + 10, T + 10), (T + 11, T + 11), (2 * T + 11, T + 10), (70, 45)]
STRIDES = [(3, 3), (4, 3), (4, 4)]
KINDS = ("noise", "flat_white", "step", "smooth", "near_black")
_cache = {}


def pair(H, W, m):
    """Image pair m of a shape and its float64 metrics, computed once."""
    key = (H, W, m)
    if key not in _cache:
        a, b = SM.images(KINDS[m % len(KINDS)], H, W, seed=m)
        _cache[key] = (a, b, SM.metrics64(a, b))
    return _cache[key]


def rows(imgs, stride):
    """[M][H, W, 3] -> device rows [M H W, stride]; what lies behind the third column is NaN and must never be read."""
    x = np.concatenate([i.reshape(-1, 3) for i in imgs])
    out = torch.full((x.shape[0], stride), float("nan"), device=DEV)
    out[:, :3] = torch.from_numpy(x).to(DEV)
    return out


def run(pred, gt, M, H, W, ssim=True, smap=True):
    """The library call itself on row tables: (sums [M,4], ssim [M,3] or None, map or None) as numpy, outputs pre-poisoned."""
    from nerf_simple_amd import _lib
    lib = _lib.lib()
    sums = torch.full((M, 4), 7.0, dtype=torch.float64, device=DEV)
    rgb = torch.full((M, 3), 7.0, dtype=torch.float64, device=DEV) if ssim else None
    mp = torch.full((M, H - 10, W - 10, 3), 7.0, device=DEV) if smap else None
    nb = int(lib.nerf_amd_image_metrics_workspace_bytes(M, H, W))
    assert nb > 0
    ws = torch.full((nb,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.check(lib.nerf_amd_image_metrics(_lib.ptr(pred), pred.stride(0), _lib.ptr(gt), gt.stride(0), _lib.ptr(sums), _lib.ptr(rgb),
                                          _lib.ptr(mp), _lib.ptr(ws), M, H, W, _lib.stream_ptr(torch.device(DEV, 0))),
               "nerf_amd_image_metrics")
    torch.cuda.synchronize()
    return sums.cpu().numpy(), None if rgb is None else rgb.cpu().numpy(), None if mp is None else mp.cpu().numpy()


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def check_against_model(sums, rgb, mp, m, want, what):
    err = float(np.abs(mp[m].astype(np.float64) - want["map"]).max())
    print(f"{what}: map error {err / SM.EPS:.2f} units of 2^-24 (bound {BOUND / SM.EPS:.0f})")
    assert err <= BOUND, (what, err / SM.EPS)
    assert float(np.abs(rgb[m] - want["ssim_rgb"]).max()) <= BOUND, what
    assert np.all(np.abs(sums[m, :3] - want["sse"]) <= SSE_REL * want["sse"]), (what, sums[m, :3], want["sse"])
    assert sums[m, 3] == want["max_gt"], what


@pytest.mark.parametrize("H,W", SHAPES, ids=lambda v: str(v))
def test_against_float64(H, W):
    for M in (1, 3):
        imgs = [pair(H, W, m) for m in range(M)]
        for ps, gs in STRIDES:
            pred, gt = rows([i[0] for i in imgs], ps), rows([i[1] for i in imgs], gs)
            sums, rgb, mp = run(pred, gt, M, H, W)
            assert mp.shape == (M, H - 10, W - 10, 3) and not np.isnan(mp).any() and not np.isnan(sums).any()
            for m in range(M):
                check_against_model(sums, rgb, mp, m, imgs[m][2], (H, W, M, ps, gs, m))


@pytest.mark.parametrize("H,W", SHAPES, ids=lambda v: str(v))
def test_identical_images_give_exactly_one(H, W):
    for kind in KINDS:
        a = SM.images(kind, H, W)[0]
        x = rows([a, a[::-1].copy()], 4)
        sums, rgb, mp = run(x, x, 2, H, W)                                  # pred IS gt: the same rows
        assert np.all(mp == np.float32(1.0)) and np.all(rgb == 1.0), (kind, H, W)
        assert np.all(sums[:, :3] == 0.0) and sums[0, 3] == a.max()
    # and through the Python call: ssim, the mean of three ones, is exactly 1
    from nerf_simple_amd.utils.metrics import image_metrics
    m = image_metrics(x, x, H, W)
    assert torch.equal(m.ssim.cpu(), torch.ones(2, dtype=torch.float64)) and bool(torch.isinf(m.psnr).all())


def windows_containing(H, W, ys, xs):
    """[H-10, W-10] bool: the positions whose 11 x 11 window holds one of the pixels."""
    hit = np.zeros((H - 10, W - 10), dtype=bool)
    for y, x in zip(ys, xs):
        hit[max(0, y - 10):y + 1, max(0, x - 10):x + 1] = True
    return hit


@pytest.mark.parametrize("H,W", [(2 * T + 11, T + 10), (70, 45)], ids=lambda v: str(v))
def test_every_pixel_is_owned_by_exactly_one_tile(H, W):
    a = SM.images("noise", H, W)[0]
    seams_y = [y for y in (T - 1, T, 2 * T - 1, 2 * T) if y < H]
    seams_x = [x for x in (T - 1, T) if x < W]
    changes = {
        "corner": ([H - 1], [W - 1]),
        "first pixel": ([0], [0]),
        "last row": ([H - 1] * W, list(range(W))),
        "last column": (list(range(H)), [W - 1] * H),
        "tile seams": ([y for y in seams_y for _ in seams_x], [x for _ in seams_y for x in seams_x]),
    }
    for what, (ys, xs) in changes.items():
        b = a.copy()
        b[ys, xs] = 1.0 - b[ys, xs]
        want = SM.metrics64(a, b)
        sums, rgb, mp = run(rows([a], 4), rows([b], 3), 1, H, W)
        assert np.all(want["sse"] > 0) and np.all(np.abs(sums[0, :3] - want["sse"]) <= SSE_REL * want["sse"]), (what, sums, want["sse"])
        hit = windows_containing(H, W, ys, xs)
        assert np.all(mp[0][~hit] == np.float32(1.0)), what
        # inside, the float64 value decides (a window that holds the pixel under its corner weight, 1.1e-6, may round to 1)
        assert np.any(mp[0][hit] != np.float32(1.0)), what
        assert float(np.abs(mp[0].astype(np.float64) - want["map"]).max()) <= BOUND, what
        assert sums[0, 3] == b.max()


def test_nan_stays_in_its_channel_and_its_image():
    H, W, M = T + 11, T + 11, 3
    imgs = [pair(H, W, m) for m in range(M)]
    clean = run(rows([i[0] for i in imgs], 4), rows([i[1] for i in imgs], 3), M, H, W)
    y, x, c, m = T - 2, T + 3, 1, 1                                         # on a tile seam's halo: four tiles stage it
    for side in ("pred", "gt"):
        a, b = [i[0].copy() for i in imgs], [i[1].copy() for i in imgs]
        (a if side == "pred" else b)[m][y, x, c] = np.nan
        sums, rgb, mp = run(rows(a, 4), rows(b, 3), M, H, W)
        hit = windows_containing(H, W, [y], [x])
        nan_map = np.zeros(mp.shape, dtype=bool)
        nan_map[m, :, :, c] = hit
        nan_sums = np.zeros((M, 4), dtype=bool)
        nan_sums[m, c] = True
        nan_sums[m, 3] = side == "gt"                                       # torch.max: a NaN in gt is the maximum
        nan_rgb = np.zeros((M, 3), dtype=bool)
        nan_rgb[m, c] = True
        assert np.array_equal(np.isnan(mp), nan_map), side
        assert np.array_equal(np.isnan(sums), nan_sums), (side, sums)
        assert np.array_equal(np.isnan(rgb), nan_rgb), (side, rgb)
        assert same_bits(mp[~nan_map], clean[2][~nan_map]) and same_bits(sums[~nan_sums], clean[0][~nan_sums])
        assert same_bits(rgb[~nan_rgb], clean[1][~nan_rgb])


def test_runs_batches_and_modes_write_the_same_bytes():
    H, W, M = 2 * T + 11, T + 10, 3
    imgs = [pair(H, W, m) for m in range(M)]
    pred, gt = rows([i[0] for i in imgs], 4), rows([i[1] for i in imgs], 3)
    first, second = run(pred, gt, M, H, W), run(pred, gt, M, H, W)
    for x, y in zip(first, second):
        assert same_bits(x, y)
    for m in range(M):                                                      # M images in one call: the M single calls
        one = run(pred[m * H * W:(m + 1) * H * W], gt[m * H * W:(m + 1) * H * W], 1, H, W)
        for x, y in zip(first, one):
            assert same_bits(x[m:m + 1], y), m
    sums, rgb, mp = run(pred, gt, M, H, W, ssim=False, smap=False)          # squared error only
    assert rgb is None and mp is None and same_bits(sums, first[0])
    sums, rgb, mp = run(pred, gt, M, H, W, ssim=False, smap=True)           # the map alone
    assert same_bits(sums, first[0]) and same_bits(mp, first[2])
    sums, rgb, mp = run(pred, gt, M, H, W, ssim=True, smap=False)
    assert same_bits(sums, first[0]) and same_bits(rgb, first[1])
    # squared error only takes any size: below one window, one pixel
    for h, w in ((10, 10), (1, 1), (3, T + 1)):
        a, b = SM.images("noise", h, w)
        want = SM.metrics64(a, b)
        sums, _, _ = run(rows([a], 4), rows([b], 3), 1, h, w, ssim=False, smap=False)
        assert np.all(np.abs(sums[0, :3] - want["sse"]) <= SSE_REL * want["sse"]) and sums[0, 3] == want["max_gt"], (h, w)


def test_python_call_shapes_and_the_reference_psnr():
    from nerf_simple_amd.utils import metrics as MT
    H, W, M = 70, 45, 3
    imgs = [pair(H, W, m) for m in range(M)]
    pred, gt = rows([i[0] for i in imgs], 4), rows([i[1] for i in imgs], 3)
    m = MT.image_metrics(pred, gt, H, W, ssim_map=True)
    raw = run(pred, gt, M, H, W)
    assert same_bits(m.sse.cpu().numpy(), raw[0][:, :3]) and same_bits(m.ssim_rgb.cpu().numpy(), raw[1])
    assert same_bits(m.map.cpu().numpy(), raw[2]) and m.mse.dtype == torch.float64 and m.mse.is_cuda
    dpsnr = 10 / math.log(10) * SSE_REL * 1.01 + 1e-12                       # what the sse bound implies for 10 log10(mse)
    for i in range(M):
        want = imgs[i][2]
        assert abs(float(m.psnr_ref[i]) - want["psnr_ref"]) <= dpsnr and abs(float(m.psnr[i]) - want["psnr"]) <= dpsnr
        assert abs(float(m.mse[i]) - want["mse"]) <= SSE_REL * want["mse"] and float(m.max_gt[i]) == want["max_gt"]
        assert abs(float(m.ssim[i]) - want["ssim"]) <= BOUND
    # the other layouts read the same rows: [M, H, W, C], and one [H, W, C] image
    m4 = MT.image_metrics(pred.view(M, H, W, 4), gt.view(M, H, W, 3), H, W)
    assert torch.equal(m4.ssim_rgb, m.ssim_rgb) and torch.equal(m4.sse, m.sse) and m4.map is None
    m1 = MT.image_metrics(pred.view(M, H, W, 4)[1], gt[H * W:2 * H * W], H, W)
    assert torch.equal(m1.ssim_rgb, m.ssim_rgb[1:2]) and torch.equal(m1.psnr_ref, m.psnr_ref[1:2])
    assert torch.equal(MT.ssim(pred, gt, H, W), m.ssim)
    assert torch.equal(MT.psnr(pred.view(M, H, W, 4), gt.view(M, H, W, 3)), m.psnr)
    no = MT.image_metrics(pred, gt, H, W, ssim=False)
    assert no.ssim is None and no.ssim_rgb is None and torch.equal(no.sse, m.sse)
    with pytest.raises(RuntimeError, match="11 x 11"):
        MT.image_metrics(pred[:100], gt[:100], 10, 10)


# ---- evaluate ----------------------------------------------------------------------------------------------------------------
BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))


@pytest.fixture(scope="module")
def trained(synthetic):
    from nerf_simple_amd.utils.dataload import RayGenerator
    from nerf_simple_amd.utils.nets import Nerf
    from nerf_simple_amd.utils.xyz import spherical_to_pose
    net = Nerf(precision="fp16").to(DEV)
    net.load_state_dict(synthetic.synthetic_state_dict(0, "structured"))
    S = 16
    cam = [S, S, synthetic.focal_from_fov(S)]
    gen = np.random.default_rng(5)
    samples = {"val": [{"img": gen.random((S, S, 3), dtype=np.float32), "transform": spherical_to_pose(4, -30, 40.0 * i)}
                       for i in range(2)]}
    return net, RayGenerator.from_samples(samples, cam, DEV), cam


def test_evaluate_is_render_view_then_image_metrics(trained):
    from nerf_simple_amd.utils import metrics as MT
    from nerf_simple_amd.utils.rendering import render_view
    net, rg, cam = trained
    out = MT.evaluate(net, rg, "val", N=16, device_rng=True)
    assert out["views"] == 2 and out["idxs"] == [0, 1] and set(out["mean"]) == {"mse", "psnr", "psnr_ref", "ssim"}
    for i in range(2):
        with torch.no_grad():
            pixels = render_view(net, rg.samples["val"][i]["transform"], cam, N=16, device_rng=True)
        m = MT.image_metrics(pixels, rg.colours["val"][i * 256:(i + 1) * 256], 16, 16)
        for key in ("mse", "psnr", "psnr_ref", "ssim"):
            assert out[key][i] == float(getattr(m, key)[0]) and math.isfinite(out[key][i]), (key, i)
        assert out["ssim_rgb"][i] == m.ssim_rgb[0].tolist()
    for key in ("mse", "psnr", "psnr_ref", "ssim"):
        assert out["mean"][key] == (out[key][0] + out[key][1]) / 2
    # a subset in another order, without SSIM
    back = MT.evaluate(net, rg, "val", [1], N=16, device_rng=True, ssim=False)
    assert back["psnr"] == [out["psnr"][1]] and "ssim" not in back and back["idxs"] == [1]
    # evaluate_views on the same poses and table is the same evaluation
    views = MT.evaluate_views(lambda pose: render_view(net, pose, cam, N=16, device_rng=True),
                              [s["transform"] for s in rg.samples["val"]], rg.colours["val"], 16, 16)
    assert all(views[k] == out[k] for k in ("mse", "psnr", "psnr_ref", "ssim", "ssim_rgb", "mean"))


def test_evaluate_through_the_acceleration_paths(trained):
    from nerf_simple_amd.utils import metrics as MT
    from nerf_simple_amd.utils.dataload import RayGenerator
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    from nerf_simple_amd.utils.proposal import ProposalVolume
    from nerf_simple_amd.utils.rendering import render_guided_view
    net, rg, cam = trained
    dense = MT.evaluate(net, rg, "val", N=16, device_rng=True)
    occ = OccupancyGrid.from_mask(torch.ones((4, 4, 4), dtype=torch.bool, device=DEV), BOUNDS, outside="live")
    masked = MT.evaluate(net, rg, "val", N=16, device_rng=True, occupancy=occ)          # an all-live grid is the dense render
    assert masked == dense
    prop = ProposalVolume(17, BOUNDS, device=DEV).update(net)
    guided = MT.evaluate(net, rg, "val", render=lambda pose: render_guided_view(net, pose, cam, 8, 16, prop, device_rng=True))
    assert guided["views"] == 2 and all(math.isfinite(v) for k in ("mse", "psnr", "psnr_ref", "ssim") for v in guided[k])
    tables = RayGenerator.from_tables(rg.rays_dataset["val"], rg.colours["val"], mode="val")
    with pytest.raises(RuntimeError, match="evaluate_views"):
        MT.evaluate(net, tables, "val", N=16)
