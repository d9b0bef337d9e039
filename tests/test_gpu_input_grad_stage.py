"""GPU tests that pin the bf16 input-gradient kernel (csrc/input_grad.hip: input_grad_kernel, rays_reduce_kernel) to its
STORED operands, element by element (tests/input_grad_stage_model.py) -- the last kernel of the training
chain that tests/test_gpu_train_chain.py stops short of.  Through the C ABI, on host-crafted and on kernel-produced buffers:

  a  exact: integer dY and weights in [-2, 2], points at the origin: dv must EQUAL G_raw + sum_l 2^l G_sin[l]
  b  exact: weights on and next to the ties of the bf16 rounding
  c  one column at a time: identity slabs, one-hot dY over all 153 (slab, column) entries: level, trig function, sign and
     coordinate of every column, each output one Jacobian term under 2^l |g| (ENC_ATOL + 2u), the other five exactly zero
  d  random integer operands at general points, every element under the derived bound
  e  the buffers the real chain produced (default and structured weights)
  f  rays mode: dv bit for bit the points-mode result on the fp32 query points; d_rays under the bound of rays_reduce
  g  rays_reduce on dyadic operands: d_rays must EQUAL the expectation
  h  a non-finite point spoils its own six outputs and nothing else
  i  two launches, identical bytes

Around the crafted operands: the seven dY layers the kernel does not read and the granules of points >= P are bf16 NaN,
features 128..255 of layer 9 the finite value 7, the parameter vector NaN outside the three weight slices, dv pre-filled with a
NaN of known payload with 64 guard floats behind it that must come back bit for bit.  A finite result therefore also proves
that nothing else is read and that the pad columns (63; 27..31) contribute zero.  Worst ratios are printed: outputs, not
tolerances."""
import numpy as np
import pytest
import torch

import input_grad_stage_model as S
from test_gpu_storage import run_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _guarded(dev, n):
    return torch.from_numpy(np.full(n + S.GUARD, S.DV_FILL_BITS, dtype=np.uint32).view(np.int32)).to(dev)


def _read_guarded(t, n, what):
    bits = t.cpu().numpy().view(np.uint32)
    assert (bits[n:] == S.DV_FILL_BITS).all(), f"{what}: the guard floats behind the output were written"
    return bits[:n].copy()


def _device_dys(dev, P, layers):
    """The device buffer of nerf_amd_train_activation_bytes(P) bytes, 0xFF everywhere but the crafted layers."""
    from nerf_simple_amd import _lib
    nbytes, n = int(_lib.lib().nerf_amd_train_activation_bytes(P)), S.layer_bytes(P)
    assert nbytes >= 10 * n
    t = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    for L, b in layers.items():
        assert b.size == n
        t[L * n:(L + 1) * n] = torch.from_numpy(b).to(dev)
    return t


def _launch(dev, P, dys, params, pts=None, rays=None, ts=None):
    """nerf_amd_input_gradients in points or rays mode -> (dv bits uint32 [6P], d_rays bits uint32 [6B] or None)."""
    from nerf_simple_amd import _lib
    lib, ptr = _lib.lib(), _lib.ptr
    par = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32)).to(dev)
    assert par.numel() == 595844
    dv = _guarded(dev, 6 * P)
    if pts is not None:
        v = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(dev)
        assert v.shape == (P, 6)
        _lib.check(lib.nerf_amd_input_gradients(ptr(dys), ptr(par), ptr(v), None, None, ptr(dv), None, P, 1,
                                                _lib.stream_ptr(dev)), "input_gradients")
        torch.cuda.synchronize()
        return _read_guarded(dv, 6 * P, "dv"), None
    B, N = ts.shape
    assert B * N == P and rays.shape == (B, 6)
    r, t = torch.from_numpy(rays).to(dev), torch.from_numpy(ts).to(dev)
    dr = _guarded(dev, 6 * B)
    _lib.check(lib.nerf_amd_input_gradients(ptr(dys), ptr(par), None, ptr(r), ptr(t), ptr(dv), ptr(dr), P, N,
                                            _lib.stream_ptr(dev)), "input_gradients")
    torch.cuda.synchronize()
    return _read_guarded(dv, 6 * P, "dv"), _read_guarded(dr, 6 * B, "d_rays")


def _run_case(dev, case):
    P = case["P"]
    dys = _device_dys(dev, P, S.craft_layers(case["dY0"], case["dY5"], case["dY9"], P))
    bits, _ = _launch(dev, P, dys, case["params"], pts=case["pts"])
    return bits.view(np.float32).reshape(P, 6)


def _assert_equal(got, want, tag):
    assert np.isfinite(got).all(), f"{tag}: a non-finite output"
    wrong = np.argwhere(got.astype(np.float64) != want)
    if wrong.size:
        detail = [(int(p), int(j), float(got[p, j]), float(want[p, j])) for p, j in wrong[:8]]
        raise AssertionError(f"{tag}: {len(wrong)} of {want.size} elements differ; first (point, output, got, want): {detail}")


def _assert_bounded(got, want, bound, tag):
    r = S.ratio(got, want, bound)
    pos, dr = float(r[:, :3].max()), float(r[:, 3:].max())
    print(f"INPUT-GRAD STAGE {tag}: worst ratio position {pos:.4f} direction {dr:.4f}")
    bad = np.argwhere(~(r <= 1))
    if bad.size:
        detail = [(int(p), int(j), float(got[p, j]), float(want[p, j]), float(bound[p, j])) for p, j in bad[:8]]
        raise AssertionError(f"{tag}: {len(bad)} elements outside the bound; first (point, output, got, want, bound): {detail}")
    return pos, dr


# ---- a, b: exact ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 15, 16, 17, 255, 257, 4099, "2 CUs 128 + 21"])
def test_exact_integers_at_the_origin(dev, P):
    """Tolerance zero.  The last size is 2 x CUs x 128 + 21 points (65,557 on 256 CUs): one 16-point group more than the
    workgroup cap of the launcher covers in one pass, so the grid-stride loop runs a second, ragged pass."""
    if isinstance(P, str):
        P = 2 * torch.cuda.get_device_properties(dev).multi_processor_count * 128 + 21
    case = S.case_integers(P, 1000 + P, origin=True)
    want, bound = S.expect(case)
    assert not bound.any() and np.array_equal(want, np.round(want)) and np.abs(want).max() > 0
    _assert_equal(_run_case(dev, case), want, f"origin P={P}")
    print(f"INPUT-GRAD STAGE origin P={P}: all {6 * P} outputs exact; largest |output| {int(np.abs(want).max())}")


@pytest.mark.parametrize("P", [17, 257])
def test_weights_are_rounded_to_nearest_even(dev, P):
    """1 + 2^-8 is a tie and goes to 1, 1 + 2^-8 + 2^-20 to 1 + 2^-7, 1 + 2^-7 + 2^-8 is a tie and goes UP to 1 + 2^-6 (and
    their negatives): the expectation uses the rounded weights and is exact (input_grad_stage_model.case_rounding)."""
    case = S.case_rounding(P, 2000 + P)
    want, bound = S.expect(case)
    assert not bound.any() and np.abs(want).max() > 0
    _assert_equal(_run_case(dev, case), want, f"rounding P={P}")


# ---- c, d, i: bounded -------------------------------------------------------------------------------------------------------
def test_one_column_at_a_time(dev):
    P = 16 * S.ENTRIES + 5
    case = S.case_onehot(P)
    want, bound = S.expect(case)
    assert set(case["entry"].tolist()) == set(range(S.ENTRIES)) and ((want != 0).sum(1) <= 1).all()
    got = _run_case(dev, case)
    try:
        _assert_bounded(got, want, bound, f"one-hot P={P}")
    except AssertionError as e:
        r = S.ratio(got, want, bound)
        cols = sorted({int(case["entry"][p]) for p in np.argwhere(~(r <= 1))[:, 0]})
        raise AssertionError(f"{e}; entries (0..62 W0, 63..125 skip slice, 126..152 C0 slice) involved: {cols}") from None


@pytest.mark.parametrize("P", [21, 600, 2405])
def test_random_integers_at_general_points(dev, P):
    case = S.case_integers(P, 3000 + P, origin=False)
    want, bound = S.expect(case)
    _assert_bounded(_run_case(dev, case), want, bound, f"integers P={P}")


def test_two_launches_give_identical_bytes(dev):
    """include/nerf_amd.h: no atomics, bit-identical results run to run."""
    case = S.case_integers(2405, 3000 + 2405, origin=False)
    a, b = _run_case(dev, case), _run_case(dev, case)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- e: kernel-produced buffers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("B,N", [(3, 7), (25, 24), (37, 65)])
def test_kernel_produced_buffers(dev, synthetic, B, N, kind):
    """The real chain (forward, compositor backward, dX chain), then the input gradient in points mode on that run's dys with
    pts = the raw columns of the stored encoder rows."""
    a = run_chain(dev, synthetic, B, N, False, kind)
    P = a["P"]
    params = S.flat_params(synthetic.synthetic_state_dict(5, kind))
    pts = np.ascontiguousarray(np.concatenate([a["posx"][:, :3], a["posd"][:, :3]], axis=1), dtype=np.float32)
    dys = torch.from_numpy(a["dys"]).to(dev)
    bits, _ = _launch(dev, P, dys, params, pts=pts)
    Wx, Wd = S.stored_weights(params)
    want, bound = S.stage(*S.stored_dys(a["dys"], P), Wx, Wd, pts)
    assert np.abs(want[:, :3]).max() > 0 and np.abs(want[:, 3:]).max() > 0
    _assert_bounded(bits.view(np.float32).reshape(P, 6), want, bound, f"chain {kind} B={B} N={N}")


# ---- f: rays mode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("craft", ["one-hot", "integers"])
@pytest.mark.parametrize("B,N", [(1, 1), (3, 7), (17, 65), (255, 3)])
def test_rays_mode(dev, oracle, B, N, craft):
    from nerf_simple_amd import _lib
    P = B * N
    case = S.case_onehot(P) if craft == "one-hot" else S.case_integers(P, 4000 + P, origin=False)
    rays, ts = S.crafted_rays(B, N, 5000 + P)
    q, _ = oracle.query_points(torch.from_numpy(rays), torch.from_numpy(ts))
    case["pts"] = np.ascontiguousarray(q.numpy(), dtype=np.float32)
    assert np.abs(case["pts"]).max() <= 4.5
    dys = _device_dys(dev, P, S.craft_layers(case["dY0"], case["dY5"], case["dY9"], P))
    dv_pts, _ = _launch(dev, P, dys, case["params"], pts=case["pts"])
    dv_rays, dr = _launch(dev, P, dys, case["params"], rays=rays, ts=ts)
    assert np.array_equal(dv_rays, dv_pts), "rays mode: dv is not the points-mode result on the fp32 query points"
    dv = dv_pts.view(np.float32).reshape(P, 6)
    _assert_bounded(dv, *S.expect(case), f"rays {craft} B={B} N={N} dv")
    want, bound = S.rays_reduce(rays, ts, dv)
    _assert_bounded(dr.view(np.float32).reshape(B, 6), want, bound, f"rays {craft} B={B} N={N} d_rays")
    # the stand-alone entry on that dv: the same bits
    lib, ptr = _lib.lib(), _lib.ptr
    r, t = torch.from_numpy(rays).to(dev), torch.from_numpy(ts).to(dev)
    dq = torch.from_numpy(dv).to(dev)
    out = _guarded(dev, 6 * B)
    _lib.check(lib.nerf_amd_query_points_backward(ptr(r), ptr(t), ptr(dq), ptr(out), B, N, _lib.stream_ptr(dev)), "qp_backward")
    torch.cuda.synchronize()
    assert np.array_equal(_read_guarded(out, 6 * B, "d_rays"), dr)


# ---- g: rays_reduce, exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 1), (255, 64), (257, 65)])
def test_rays_reduce_on_dyadic_operands(dev, B, N):
    """Integer d_q in [-2, 2], ts in multiples of 1/8 in [2, 6], directions +-2^k e_m (k = -2 .. 2): |d| = 2^k and d_hat =
    +-e_m exactly, every product and partial sum is a multiple of 1/8 below 2^12, so d_rays must EQUAL
    [sum dx, sum t dx + (g - e_m g_m) / 2^k]."""
    from nerf_simple_amd import _lib
    rng = np.random.Generator(np.random.PCG64(6000 + B))
    d_q = rng.integers(-2, 3, size=(B, N, 6)).astype(np.float32)
    ts = (rng.integers(16, 49, size=(B, N)) / 8.0).astype(np.float32)
    m, k, s = rng.integers(0, 3, size=B), rng.integers(-2, 3, size=B), rng.choice([-1.0, 1.0], size=B)
    rays = rng.uniform(-2, 2, size=(B, 6)).astype(np.float32)
    rays[:, 3:] = 0
    rays[np.arange(B), 3 + m] = (s * 2.0 ** k).astype(np.float32)
    dx, du = d_q[:, :, :3].astype(np.float64), d_q[:, :, 3:].astype(np.float64)
    g = du.sum(1)
    g[np.arange(B), m] = 0                                             # g - e_m g_m
    want = np.concatenate([dx.sum(1), (ts.astype(np.float64)[:, :, None] * dx).sum(1) + g / 2.0 ** k[:, None]], axis=1)
    model, _ = S.rays_reduce(rays, ts, d_q.reshape(B * N, 6))
    assert np.array_equal(model, want) and np.abs(want[:, 3:]).max() > 0
    lib, ptr = _lib.lib(), _lib.ptr
    out = _guarded(dev, 6 * B)
    r, t, q = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rays, ts, d_q))
    _lib.check(lib.nerf_amd_query_points_backward(ptr(r), ptr(t), ptr(q), ptr(out), B, N, _lib.stream_ptr(dev)), "qp_backward")
    torch.cuda.synchronize()
    _assert_equal(_read_guarded(out, 6 * B, "d_rays").view(np.float32).reshape(B, 6), want, f"rays_reduce B={B} N={N}")


# ---- h: a non-finite point stays alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_point_stays_alone(dev, value):
    """One point of a 16-point group carries NaN (Inf) in dY0 -- and in dY9, or its three direction outputs, which no product
    with dY0 enters, would rightly stay finite: all six of its outputs are non-finite, every other point (the other fifteen
    of its group included) has the bits of the clean run.  With the value in dY0 alone the point's direction outputs keep the
    clean run's bits as well.  Points: one in a full group, one in the ragged last group."""
    P = 600
    case = S.case_integers(P, 7000, origin=False)
    clean = _run_case(dev, case).view(np.uint32)
    for p, with_dy9 in ((16 * 7 + 3, True), (P - 3, True), (16 * 7 + 3, False)):
        bad = dict(case)
        bad["dY0"], bad["dY9"] = case["dY0"].copy(), case["dY9"].copy()
        bad["dY0"][p, 5] = value
        if with_dy9:
            bad["dY9"][p, 7] = value
        got = _run_case(dev, bad)
        bits = got.view(np.uint32)
        others = np.arange(P) != p
        assert np.array_equal(bits[others], clean[others]), (p, with_dy9)
        assert not np.isfinite(got[p, :3]).any(), (p, got[p])
        if with_dy9:
            assert not np.isfinite(got[p, 3:]).any(), (p, got[p])
        else:
            assert np.array_equal(bits[p, 3:], clean[p, 3:]), (p, got[p])
