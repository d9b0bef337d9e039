"""Density grids and marching cubes on the GPU (csrc/density.hip, csrc/marching_cubes.hip, utils/mesh.py).

sigma of the sigma-only kernel must equal column 3 of nerf_amd_mlp_forward bit for bit (same packed image, same
arithmetic); the mesh must equal the numpy restatement tests/mesh_model.py (vertices and faces exactly, normals to 1e-6).
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import mesh_model as M

pytestmark = pytest.mark.gpu

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
UNIT = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    return _lib.lib()


def stream(dev):
    from nerf_simple_amd import _lib
    return _lib.stream_ptr(dev)


def f3(a):
    return (ctypes.c_float * 3)(*[float(x) for x in a])


def make_net(dev, kind, precision=None):
    from nerf_simple_amd.utils import synthetic
    from nerf_simple_amd.utils.nets import Nerf
    net = Nerf(precision=precision).to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, kind))
    return net


def torch_grid_points(R, bounds, dev):
    """the grid points formed by torch: lo + arange(R) * step in float32, C order, direction (0, 0, 1)"""
    from nerf_simple_amd.utils import mesh
    lo, step = mesh.grid_axes(R, bounds)
    axes = [torch.tensor(lo[a], device=dev) + torch.arange(R[a], dtype=torch.float32, device=dev) * torch.tensor(step[a], device=dev)
            for a in range(3)]
    X, Y, Z = torch.meshgrid(*axes, indexing="ij")
    p = torch.stack([X, Y, Z], -1).reshape(-1, 3)
    return torch.cat([p, torch.zeros_like(p[:, :2]), torch.ones_like(p[:, :1])], 1).contiguous()


def mlp_sigma(lib, net, pts6, code, dev):
    from nerf_simple_amd import _lib
    out = torch.empty((pts6.shape[0], 4), dtype=torch.float32, device=dev)
    _lib.check(lib.nerf_amd_mlp_forward(_lib.ptr(pts6), _lib.ptr(net.packed_weights(code)), _lib.ptr(out), pts6.shape[0], code,
                                        stream(dev)), "nerf_amd_mlp_forward")
    return out[:, 3].contiguous()


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. bit for bit against the points-mode forward ----------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("R", [(37, 41, 29), (256, 256, 256)])
def test_density_equals_forward_sigma_bit_for_bit(dev, lib, precision, kind, R):
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils import mesh
    net = make_net(dev, kind, precision)
    code = _lib.precision_code(precision)
    pts6 = torch_grid_points(R, BOUNDS, dev)
    want = mlp_sigma(lib, net, pts6, code, dev)
    lo, step = mesh.grid_axes(R, BOUNDS)
    grid = torch.empty(R, dtype=torch.float32, device=dev)
    assert lib.nerf_amd_density_grid(f3(lo), f3(step), *R, _lib.ptr(net.packed_weights(code)), code, _lib.ptr(grid), stream(dev)) == 0
    # points mode: the [P,6] table, a [P,3] one, and rows of stride 7
    pts3 = pts6[:, :3].contiguous()
    pts7 = torch.cat([pts3, torch.full((pts3.shape[0], 4), 7.0, device=dev)], 1).contiguous()
    got = {}
    for name, p, stride in (("p6", pts6, 6), ("p3", pts3, 3), ("p7", pts7, 7)):
        s = torch.empty(p.shape[0], dtype=torch.float32, device=dev)
        assert lib.nerf_amd_density_forward(_lib.ptr(p), stride, _lib.ptr(net.packed_weights(code)), code, _lib.ptr(s),
                                            p.shape[0], stream(dev)) == 0
        got[name] = s
    with torch.no_grad():
        got["module"] = net.density(pts3)
    got["grid_api"] = mesh.density_grid(net, R, BOUNDS)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    assert torch.equal(bits(grid.view(-1)), bits(want)), (precision, kind, R)
    for name, s in got.items():
        assert torch.equal(bits(s.view(-1)), bits(want)), (name, precision, kind, R)
    from nerf_simple_amd.utils.nets import packed_status
    assert packed_status(net.packed_weights(code), code) == 0


# ---- 2. against the oracle, and the fp32 / other-size paths ----------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_density_grid_within_the_error_model(dev, precision, synthetic):
    import error_model as E
    from nerf_simple_amd.utils import mesh
    R = (24, 24, 24)
    for kind in ("default", "structured"):
        sd = synthetic.synthetic_state_dict(0, kind)
        net = make_net(dev, kind, precision)
        got = mesh.density_grid(net, R, BOUNDS).view(-1).double().cpu()
        pts = torch_grid_points(R, BOUNDS, dev).cpu()
        truth = E.f64_forward(sd, pts)[:, 3]
        emu = E.emulated_forward(sd, pts, precision)[:, 3].double()
        # the error model's rule (tests/error_model.py): per output, max norm scaled by max(1, |truth|)
        err, bound = E.scaled_err(got.numpy(), truth.numpy()), E.FACTOR_16 * E.scaled_err(emu.numpy(), truth.numpy()) + E.ULP_FLOOR
        assert err <= bound, (kind, precision, err, bound)


def test_fp32_and_other_sizes_equal_forward_bit_for_bit(dev, synthetic):
    from nerf_simple_amd.utils import mesh
    from nerf_simple_amd.utils.nets import Nerf
    R = (24, 24, 24)
    pts6 = torch_grid_points(R, BOUNDS, dev)
    net32 = make_net(dev, "structured", "fp32")
    torch.manual_seed(0)
    small = Nerf(6, 2, 128).to(dev)
    for net in (net32, small):
        with torch.no_grad():
            want = net(pts6)[:, 3].contiguous()
            pts3 = pts6[:, :3].contiguous()
            dens = net.density(pts3)
        grid = mesh.density_grid(net, R, BOUNDS)
        assert torch.equal(bits(grid.view(-1)), bits(want))
        assert torch.equal(bits(dens), bits(want))
    # fp32 requested of a 16-bit module takes the same path
    net16 = make_net(dev, "structured", "fp16")
    assert torch.equal(bits(mesh.density_grid(net16, R, BOUNDS, precision="fp32").view(-1)), bits(mesh.density_grid(net32, R, BOUNDS).view(-1)))


def test_range_warning_iff_forward_would_raise(dev):
    from nerf_simple_amd.utils import mesh
    net = make_net(dev, "default", "bf16")
    R = (5, 6, 7)
    for bounds in (UNIT, ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0001)), BOUNDS, ((-0.5, -1.0, -1.0), (0.5, 0.25, 1.0)),
                   ((0.9, -1.0, -1.0), (-1.0, 0.3, 0.4))):
        p = torch_grid_points(R, bounds, dev)
        want = bool((p < -1).any() or (p > 1).any())           # what Nerf.forward on these points checks (utils/xyz.py:8-9)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            mesh.density_grid(net, R, bounds)
        hits = [w for w in rec if "input not in range -1,1" in str(w.message)]
        assert len(hits) == (1 if want else 0), bounds


# ---- 3. range guard ---------------------------------------------------------------------------------------------------
def high_gain_state_dict(synthetic, gain):
    """The structured weights with the first hidden layer scaled up by ``gain`` and the second layer's weights scaled down by
    it: the same function in exact arithmetic (ReLU is positively homogeneous), hidden activations far beyond fp16's 65504
    for gain = 1e5, every weight finite in fp16."""
    sd = {k: v.clone() for k, v in synthetic.synthetic_state_dict(0, "structured").items()}
    sd["layers_0.0.weight"] *= gain
    sd["layers_0.0.bias"] *= gain
    sd["layers_0.2.weight"] /= gain
    return sd


def test_fp16_overflow_demotes_to_bf16(dev, lib, synthetic):
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils import mesh
    from nerf_simple_amd.utils.nets import Nerf, packed_status
    sd = high_gain_state_dict(synthetic, 1e5)
    R = (24, 24, 24)
    # the raw kernel sets the status word
    raw = Nerf(precision="fp16").to(dev)
    raw.load_state_dict(sd)
    lo, step = mesh.grid_axes(R, UNIT)
    s = torch.empty(R, dtype=torch.float32, device=dev)
    assert lib.nerf_amd_density_grid(f3(lo), f3(step), *R, _lib.ptr(raw.packed_weights(_lib.FP16)), _lib.FP16, _lib.ptr(s),
                                     stream(dev)) == 0
    assert packed_status(raw.packed_weights(_lib.FP16), _lib.FP16) & _lib.STATUS_NONFINITE
    # the host side: one warning, the bf16 volume
    net = Nerf(precision="fp16").to(dev)
    net.load_state_dict(sd)
    ref = Nerf(precision="bf16").to(dev)
    ref.load_state_dict(sd)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = mesh.density_grid(net, R, UNIT)
    hits = [w for w in rec if "fp16 MFMA operands left their range" in str(w.message)]
    assert len(hits) == 1
    want = mesh.density_grid(ref, R, UNIT)
    assert torch.equal(bits(got), bits(want))
    assert packed_status(ref.packed_weights(_lib.BF16), _lib.BF16) == 0


def test_nan_weights_follow_the_reference(dev, synthetic, oracle):
    from nerf_simple_amd.utils import mesh
    from nerf_simple_amd.utils.nets import Nerf
    sd = {k: v.clone() for k, v in synthetic.synthetic_state_dict(0, "structured").items()}
    sd["layers_0.0.weight"][3, 5] = float("nan")
    R = (12, 10, 9)
    net = Nerf(precision="bf16").to(dev)
    net.load_state_dict(sd)
    ref = Nerf(precision="fp32").to(dev)
    ref.load_state_dict(sd)
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        got = mesh.density_grid(net, R, UNIT).cpu().numpy()
    want = mesh.density_grid(ref, R, UNIT).cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True)
    pts = torch_grid_points(R, UNIT, dev).cpu()
    with torch.no_grad():
        o = oracle.nerf_forward(sd, pts)[:, 3].numpy()
    assert np.array_equal(np.isnan(got.reshape(-1)), np.isnan(o))


# ---- 4. marching cubes against the numpy restatement ---------------------------------------------------------------
def gpu_mesh(field, level, bounds, dev):
    from nerf_simple_amd.utils import mesh
    v, f, n = mesh.marching_cubes(torch.from_numpy(field).to(dev), level, bounds)
    return v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()


def assert_same_mesh(field, level, bounds, dev):
    lo, step = np.asarray(bounds[0], np.float32), M.grid_step(bounds[0], bounds[1], field.shape)
    want = M.marching_cubes(field, level, lo, step)
    got = gpu_mesh(field, level, bounds, dev)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.allclose(got[2], want[2], rtol=0, atol=1e-6)
    return got


@pytest.mark.parametrize("R", [(64, 64, 64), (97, 80, 71)])
def test_sphere(dev, R):
    field, _ = M.sphere_field(R)
    v, f, n = assert_same_mesh(field, 0.0, UNIT, dev)
    assert M.directed_edges_closed(f)
    assert M.euler_characteristic(v, f) == 2
    area, vol = M.area_and_volume(v, f)
    r = 0.6
    assert abs(area / (4 * np.pi * r * r) - 1) < 0.01
    assert vol > 0 and abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.01
    # repeated runs: the same bytes
    again = gpu_mesh(field, 0.0, UNIT, dev)
    for a, b in zip((v, f, n), again):
        assert a.tobytes() == b.tobytes()


def test_torus_and_gaussians(dev):
    field, _ = M.torus_field((72, 64, 56))
    v, f, _ = assert_same_mesh(field, 0.0, UNIT, dev)
    assert M.directed_edges_closed(f) and M.euler_characteristic(v, f) == 0
    field, _ = M.gaussians_field((61, 50, 57), seed=3)
    v, f, _ = assert_same_mesh(field, 0.0, UNIT, dev)
    assert M.directed_edges_closed(f)
    field, _ = M.gaussians_field((40, 40, 40), seed=5)
    assert_same_mesh(field, 0.25, BOUNDS, dev)


# ---- 5. edges -------------------------------------------------------------------------------------------------------
def test_empty_and_tied_fields(dev):
    const = np.full((9, 8, 7), 2.0, np.float32)
    for level in (2.0, 1.0, 3.0):
        v, f, n = gpu_mesh(const, level, UNIT, dev)
        assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    field, _ = M.sphere_field((20, 20, 20))
    for level in (-10.0, 10.0):
        v, f, _ = gpu_mesh(field, level, UNIT, dev)
        assert v.shape[0] == 0 and f.shape[0] == 0
    # sigma == level counts as outside: a single cell with one corner above and one exactly at the level
    cell = np.zeros((2, 2, 2), np.float32)
    cell[0, 0, 0] = 1.0
    cell[1, 1, 1] = 0.5
    v, f, _ = assert_same_mesh(cell, 0.5, UNIT, dev)
    assert v.shape == (3, 3) and f.shape == (1, 3)
    # quantised fields with many exact ties
    rng = np.random.default_rng(0)
    q = rng.integers(0, 4, size=(13, 11, 12)).astype(np.float32)
    assert_same_mesh(q, 2.0, UNIT, dev)


def test_non_finite_corners(dev):
    field, _ = M.gaussians_field((30, 28, 26), seed=1)
    rng = np.random.default_rng(2)
    flat = field.reshape(-1)
    idx = rng.choice(flat.size, 400, replace=False)
    flat[idx[:150]] = np.nan
    flat[idx[150:300]] = np.inf
    flat[idx[300:]] = -np.inf
    assert_same_mesh(field, 0.0, UNIT, dev)


def test_single_cell_and_errors(dev, lib):
    from nerf_simple_amd import _lib
    cell = np.zeros((2, 2, 2), np.float32)
    cell[0, 0, 0] = 1.0
    v, f, n = assert_same_mesh(cell, 0.5, UNIT, dev)
    assert v.shape == (3, 3) and f.shape == (1, 3)
    vol = torch.zeros((4, 4, 4), device=dev)
    ws = torch.empty(int(lib.nerf_amd_marching_cubes_workspace_bytes(4, 4, 4)), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    lvl = ctypes.c_float(0.0)
    EINVAL, EUNSUP = -1, -2
    assert lib.nerf_amd_marching_cubes_workspace_bytes(1, 4, 4) == EINVAL
    assert lib.nerf_amd_marching_cubes_count(_lib.ptr(vol), 4, 1, 4, lvl, _lib.ptr(ws), _lib.ptr(counts), stream(dev)) == EINVAL
    assert lib.nerf_amd_marching_cubes_count(None, 4, 4, 4, lvl, _lib.ptr(ws), _lib.ptr(counts), stream(dev)) == EINVAL
    assert lib.nerf_amd_marching_cubes_count(_lib.ptr(vol), 4, 4, 4, lvl, None, _lib.ptr(counts), stream(dev)) == EINVAL
    assert lib.nerf_amd_marching_cubes_count(_lib.ptr(vol), 4, 4, 4, lvl, _lib.ptr(ws), None, stream(dev)) == EINVAL
    lo, st = f3((0, 0, 0)), f3((1, 1, 1))
    out = torch.empty((8, 3), device=dev)
    faces = torch.empty((8, 3), dtype=torch.int32, device=dev)
    assert lib.nerf_amd_marching_cubes_emit(_lib.ptr(vol), 4, 4, 1, lvl, lo, st, _lib.ptr(ws), _lib.ptr(out), None, _lib.ptr(faces),
                                            8, 8, stream(dev)) == EINVAL
    assert lib.nerf_amd_marching_cubes_emit(_lib.ptr(vol), 4, 4, 4, lvl, None, st, _lib.ptr(ws), _lib.ptr(out), None,
                                            _lib.ptr(faces), 8, 8, stream(dev)) == EINVAL
    assert lib.nerf_amd_marching_cubes_emit(_lib.ptr(vol), 4, 4, 4, lvl, lo, st, _lib.ptr(ws), None, None, _lib.ptr(faces), 8, 8,
                                            stream(dev)) == EINVAL
    assert lib.nerf_amd_marching_cubes_emit(_lib.ptr(vol), 4, 4, 4, lvl, lo, st, _lib.ptr(ws), _lib.ptr(out), None, None, 8, 8,
                                            stream(dev)) == EINVAL
    assert lib.nerf_amd_marching_cubes_emit(_lib.ptr(vol), 4, 4, 4, lvl, lo, st, _lib.ptr(ws), _lib.ptr(out), None,
                                            _lib.ptr(faces), 1 << 31, 8, stream(dev)) == EINVAL
    # density entries
    net = make_net(dev, "default", "bf16")
    pk = _lib.ptr(net.packed_weights(_lib.BF16))
    s = torch.empty(64, device=dev)
    assert lib.nerf_amd_density_grid(lo, st, 4, 4, 4, pk, _lib.F32, _lib.ptr(s), stream(dev)) == EUNSUP
    assert lib.nerf_amd_density_grid(lo, st, 4, 1, 16, pk, _lib.BF16, _lib.ptr(s), stream(dev)) == EINVAL
    assert lib.nerf_amd_density_grid(lo, st, 4, 4, 1 << 25, pk, _lib.BF16, _lib.ptr(s), stream(dev)) == EINVAL
    assert lib.nerf_amd_density_grid(None, st, 4, 4, 4, pk, _lib.BF16, _lib.ptr(s), stream(dev)) == EINVAL
    assert lib.nerf_amd_density_grid(lo, st, 4, 4, 4, None, _lib.BF16, _lib.ptr(s), stream(dev)) == EINVAL
    assert lib.nerf_amd_density_grid(lo, st, 4, 4, 4, pk, 7, _lib.ptr(s), stream(dev)) == EINVAL
    pts = torch.zeros((64, 3), device=dev)
    assert lib.nerf_amd_density_forward(_lib.ptr(pts), 2, pk, _lib.BF16, _lib.ptr(s), 64, stream(dev)) == EINVAL
    assert lib.nerf_amd_density_forward(_lib.ptr(pts), 3, pk, _lib.F32, _lib.ptr(s), 64, stream(dev)) == EUNSUP
    assert lib.nerf_amd_density_forward(None, 3, pk, _lib.BF16, _lib.ptr(s), 64, stream(dev)) == EINVAL
    assert lib.nerf_amd_density_forward(_lib.ptr(pts), 3, pk, _lib.BF16, None, 64, stream(dev)) == EINVAL
    assert lib.nerf_amd_grid_points(lo, st, 4, 4, 4, 60, 5, _lib.ptr(out), stream(dev)) == EINVAL
    assert lib.nerf_amd_grid_points(lo, st, 4, 4, 4, 0, 4, None, stream(dev)) == EINVAL
    torch.cuda.synchronize()


def test_capacities_are_never_exceeded(dev, lib):
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils import mesh
    field, _ = M.sphere_field((24, 22, 20))
    vol = torch.from_numpy(field).to(dev)
    v_all, f_all, n_all = mesh.marching_cubes(vol, 0.0, UNIT)
    V, F = v_all.shape[0], f_all.shape[0]
    R = field.shape
    lo, step = mesh.grid_axes(R, UNIT)
    ws = torch.empty(int(lib.nerf_amd_marching_cubes_workspace_bytes(*R)), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    lvl = ctypes.c_float(0.0)
    assert lib.nerf_amd_marching_cubes_count(_lib.ptr(vol), *R, lvl, _lib.ptr(ws), _lib.ptr(counts), stream(dev)) == 0
    assert counts.cpu().tolist() == [V, F]
    PAD = 64
    for cv, cf in ((V // 3, F // 2), (0, F - 1), (V - 1, 0), (V, F)):
        verts = torch.full((cv + PAD, 3), 1234.5, device=dev)
        normals = torch.full((cv + PAD, 3), -99.0, device=dev)
        faces = torch.full((cf + PAD, 3), -7, dtype=torch.int32, device=dev)
        assert lib.nerf_amd_marching_cubes_emit(_lib.ptr(vol), *R, lvl, f3(lo), f3(step), _lib.ptr(ws), _lib.ptr(verts),
                                                _lib.ptr(normals), _lib.ptr(faces), cv, cf, stream(dev)) == 0
        assert torch.equal(verts[:cv], v_all[:cv]) and torch.equal(normals[:cv], n_all[:cv]) and torch.equal(faces[:cf], f_all[:cf])
        assert (verts[cv:] == 1234.5).all() and (normals[cv:] == -99.0).all() and (faces[cf:] == -7).all()


# ---- 6. composition ----------------------------------------------------------------------------------------------------
def test_extract_mesh_composes(dev, tmp_path):
    from nerf_simple_amd.utils import mesh
    net = make_net(dev, "structured", "fp16")
    R = (48, 44, 40)
    vol = mesh.density_grid(net, R, BOUNDS)
    level = float(vol.view(-1).median())
    v, f, n = mesh.marching_cubes(vol, level, BOUNDS)
    assert f.shape[0] > 100
    v2, f2, n2, rgb = mesh.extract_mesh(net, R, level, BOUNDS, colors=True)
    assert torch.equal(v, v2) and torch.equal(f, f2) and torch.equal(n, n2)
    with torch.no_grad():
        want = net(torch.cat([v, -n], 1))[:, :3]
    assert torch.equal(bits(rgb), bits(want))
    v3, f3_, n3 = mesh.extract_mesh(net, R, level, BOUNDS)
    assert torch.equal(v, v3) and torch.equal(f, f3_)
    # the whole path end to end into a file
    path = mesh.save_ply(str(tmp_path / "m.ply"), v2, f2, n2, torch.sigmoid(rgb))
    assert open(path, "rb").read(3) == b"ply"


def test_density_gradients_are_forwards(dev):
    net = make_net(dev, "structured", "bf16")
    g = torch.Generator().manual_seed(4)
    x = (torch.rand(500, 3, generator=g) * 2 - 1).to(dev)
    a = x.clone().requires_grad_()
    s = net.density(a)
    s.pow(2).sum().backward()
    b = x.clone().requires_grad_()
    v = torch.cat([b, torch.zeros_like(b[:, :2]), torch.ones_like(b[:, :1])], 1)
    net(v)[:, 3].pow(2).sum().backward()
    assert torch.equal(a.grad, b.grad)
    # and without gradients the kernel path gives the same sigma as forward's column 3
    with torch.no_grad():
        assert torch.equal(bits(net.density(x)), bits(net(torch.cat([x, torch.zeros_like(x[:, :2]), torch.ones_like(x[:, :1])], 1))[:, 3]))
