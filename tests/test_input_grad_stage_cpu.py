"""CPU tests of tests/input_grad_stage_model.py: the evidence that the per-element rule which tests/test_gpu_input_grad_stage.py
applies to the bf16 input-gradient kernel passes correct arithmetic on the committed cases and rejects every defect such a
kernel is prone to -- and the reason the rule exists: the end-to-end rule of tests/input_grad_model.py (max norm over the whole
[P, 6] tensor, allowance FACTOR_16 x the emulation's own error) cannot see the direction outputs at all.

``emulate`` is an fp32 numpy rendition of csrc/input_grad.hip input_grad_kernel on the buffers themselves (the flat parameter
vector and the point-blocked bf16 buffer): weights staged and rounded to bf16, fp32 products summed one 32-wide k-step at a
time, float32 sin / cos on the exactly scaled argument, one rounding per Jacobian term, the terms added per lane group in
column order and the four groups by the kernel's butterfly.  ``fault`` plants one defect."""
import numpy as np
import pytest
import torch

import input_grad_model as IG
import input_grad_stage_model as S
import train_chain_model as C

F32 = np.float32


def _round_weights(w, truncate):
    if truncate:
        return (np.ascontiguousarray(w, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
    return C.round_bf16(w)


def emulate(params, dys, pts, P, fault=None):
    params = np.asarray(params, dtype=F32)
    dY = C.decode_bf16_layers(dys, P)
    dY0, dY5, dY9 = dY[0], dY[5], dY[9][:, :128]
    if fault == "drop_dy5":
        dY5 = np.zeros_like(dY5)
    o0, o5, o9 = (C.OFFSETS[n][0] for n in ("layers_0.0.weight", "skip_conn_layer.0.weight", "color_fc.0.weight"))
    pad = fault == "pad_column"
    ncx, ncd = (64, 32) if pad else (S.NX, S.ND)
    k, kd = np.arange(256)[None, :], np.arange(128)[None, :]
    cx, cd = np.arange(ncx)[:, None], np.arange(ncd)[:, None]
    # the staging loop: [c][k] images; a column that is not staged is zero
    wx, wd = np.zeros((64, 512), F32), np.zeros((32, 128), F32)
    wx[:ncx, :256] = params[o0 + k * 63 + cx]
    wx[:ncx, 256:] = params[o5 + k * 319 + (255 if fault == "skip_255" else 256) + cx]
    wd[:ncd] = params[o9 + kd * 283 + (255 if fault == "c0_255" else 256) + cd]
    wx, wd = _round_weights(wx, fault == "truncate"), _round_weights(wd, fault == "truncate")

    def product(b, w):
        acc = np.zeros((P, w.shape[0]), F32)
        with np.errstate(invalid="ignore"):
            for s in range(b.shape[1] // 32):
                acc = acc + b[:, 32 * s:32 * s + 32] @ w[:, 32 * s:32 * s + 32].T
        return acc

    gx, gd = product(np.concatenate([dY0, dY5], axis=1), wx), product(dY9, wd)
    pts = np.asarray(pts, dtype=F32)
    gv = np.zeros((4, P, 6), F32)                                     # one partial per lane group

    def term(x, level, trig, g):
        if fault == "swap_trig":
            trig ^= 1
        if fault == "level_plus_one":
            level += 1
        a = np.ldexp(x, level).astype(F32)
        r = (np.sin(a) if fault == "sin_sign" else -np.sin(a)) if trig else np.cos(a)
        with np.errstate(invalid="ignore"):
            return np.ldexp(r.astype(F32), level).astype(F32) * g

    for G, base, L, ncol in ((gx, 0, S.LP, ncx), (gd, 3, S.LD, ncd)):
        for c in range(ncol):
            grp = (c % 16) // 4
            if c < 3:
                if fault != "drop_raw":
                    gv[grp, :, base + c] += G[:, c]
                continue
            kk, idx = divmod(c - 3, 2 * L)
            src = min(base + kk, 5)                                   # (a pad column computes coordinate 3: past the array)
            dst = base + (kk + 1) % 3 if (fault == "permute" and kk < 3) else src
            gv[grp, :, dst] += term(pts[:, src], idx >> 1, idx & 1, G[:, c])
    with np.errstate(invalid="ignore"):
        out = (gv[0] + gv[1]) + (gv[2] + gv[3])
    if fault == "zero_direction":
        out[:, 3:] = 0
    if fault == "swap_pairs":
        out = out[:, [1, 0, 3, 2, 5, 4]]
    return out


FAULTS = {
    "drop_raw": "raw column dropped",
    "swap_trig": "sin and cos swapped",
    "level_plus_one": "level off by one",
    "permute": "coordinates permuted",
    "sin_sign": "sign of the sin term flipped",
    "drop_dy5": "the dY5 half (k >= 256) dropped",
    "skip_255": "skip-weight column offset 255 instead of 256",
    "c0_255": "C0 column offset 255 instead of 256",
    "pad_column": "pad column 63 (27..31) staged and used as a weight column",
    "zero_direction": "direction output zeroed",
    "truncate": "weights truncated to bf16 instead of rounded to nearest even",
    "swap_pairs": "output pairs written in swapped order",
}

# the committed cases at the smallest sizes that still have a ragged group and a second tile
CASES = {
    "a origin": lambda: S.case_integers(257, 1, origin=True),
    "b rounding": lambda: S.case_rounding(257, 2),
    "c one-hot": lambda: S.case_onehot(4 * S.ENTRIES + 5),
    "d integers": lambda: S.case_integers(600, 3, origin=False),
}
_cache = {}


def _case(name):
    if name not in _cache:
        case = CASES[name]()
        case["dys"] = S.craft_dys(case["dY0"], case["dY5"], case["dY9"], case["P"])
        case["want"], case["bound"] = S.expect(case)
        _cache[name] = case
    return _cache[name]


def _worst(case, fault=None):
    got = emulate(case["params"], case["dys"], case["pts"], case["P"], fault)
    return float(S.ratio(got, case["want"], case["bound"]).max()), got


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulation_stays_inside_the_bound(name):
    """The inputs and the bounds are ones a correct fp32 evaluation stays within; the exact cases are met exactly."""
    case = _case(name)
    worst, got = _worst(case)
    print(f"CPU {name}: worst ratio {worst:.4f}")
    assert np.abs(case["want"]).max() > 0
    if name[0] in "ab":
        assert not case["bound"].any() and np.array_equal(got.astype(np.float64), case["want"])
    assert worst <= 1, worst


def test_exact_cases_agree_with_the_general_model():
    """exact_at_origin (integer arithmetic on the sin columns) is the general float64 model at pts = 0."""
    for name in ("a origin", "b rounding"):
        case = _case(name)
        Wx, Wd = S.stored_weights(case["params"])
        want, _ = S.stage(case["dY0"], case["dY5"], case["dY9"], Wx, Wd, case["pts"])
        assert np.array_equal(want, case["want"]), name
    assert np.array_equal(np.unique(np.abs(S.stored_weights(_case("b rounding")["params"])[0])),
                          np.concatenate([[0.0], S.ROUNDED_WEIGHTS]))


def test_one_hot_case_covers_every_column_and_its_bound_is_one_term():
    case = _case("c one-hot")
    assert set(case["entry"].tolist()) == set(range(153))
    want, bound = case["want"], case["bound"]
    assert ((want != 0).sum(1) <= 1).all() and ((bound != 0).sum(1) <= 1).all()
    # entry 3 + 20 j + 2 l + t of the position, at level l: 2^l |g| (ENC_ATOL + 2u), and 0 for a raw column
    p = int(np.flatnonzero(case["entry"] == 3 + 20 * 1 + 2 * 9 + 1)[0])
    one_term = 512.0 * abs(float(case["value"][p])) * (S.ENC_ATOL + 2 * S.U)
    assert bound[p, 1] == pytest.approx(one_term, rel=1e-14) and not np.delete(bound[p], 1).any()
    assert not bound[case["entry"] < 3].any() and not bound[case["entry"] == 126].any()


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_is_rejected(fault):
    """Every defect is rejected by at least one committed case (printed: which ones, and the ratio)."""
    caught = {}
    for name in sorted(CASES):
        worst, _ = _worst(_case(name), fault)
        if not worst <= 1:
            caught[name] = worst
    print(f"FAULT {fault} ({FAULTS[fault]}): {caught}")
    assert caught, fault


def test_crafted_encoder_is_the_model_encoder():
    """craft_layer writes what train_chain_model.encode_bf16_layers writes; the other seven layers are bf16 NaN."""
    P = 300
    case = S.case_integers(P, 5, origin=False)
    buf = S.craft_dys(case["dY0"], case["dY5"], case["dY9"], P)
    layers = [np.zeros((P, 256), F32) for _ in range(10)]
    layers[0], layers[5] = case["dY0"], case["dY5"]
    layers[9] = np.concatenate([case["dY9"], np.full((P, 128), 7.0, F32)], axis=1)
    ref = C.encode_bf16_layers(layers, P)
    n = S.layer_bytes(P)
    assert buf.size == ref.size == 10 * n
    for L in range(10):
        if L in (0, 5, 9):
            assert np.array_equal(buf[L * n:(L + 1) * n], ref[L * n:(L + 1) * n]), L
        else:
            assert (buf[L * n:(L + 1) * n] == 0xFF).all(), L
    dY0, dY5, dY9 = S.stored_dys(buf, P)
    assert np.array_equal(dY0, case["dY0"]) and np.array_equal(dY5, case["dY5"]) and np.array_equal(dY9, case["dY9"])
    # the parameter vector: NaN outside the three slices
    p = case["params"]
    assert np.isfinite(p).sum() == 256 * 63 * 2 + 128 * 27
    assert np.isfinite(S._mat(p, "skip_conn_layer.0.weight")[:, 256:]).all()


# ---- rays_reduce ------------------------------------------------------------------------------------------------------------
def _reduce_f32(rays, ts, d_q):
    """rays_reduce_kernel in fp32 numpy (separate roundings; the compiler may contract some into fmas)."""
    B, N = ts.shape
    q = d_q.reshape(B, N, 6)
    go, gd, gu = np.zeros((B, 3), F32), np.zeros((B, 3), F32), np.zeros((B, 3), F32)
    for n in range(N):
        go = go + q[:, n, :3]
        gd = (ts[:, n, None].astype(np.float64) * q[:, n, :3] + gd).astype(F32)          # one rounding: an fma
        gu = gu + q[:, n, 3:]
    d = rays[:, 3:]
    s = (d[:, 0] * d[:, 0]).astype(F32)
    s = (d[:, 1].astype(np.float64) * d[:, 1] + s).astype(F32)
    s = (d[:, 2].astype(np.float64) * d[:, 2] + s).astype(F32)
    nrm = np.sqrt(s).astype(F32)[:, None]
    u = (d / nrm).astype(F32)
    ug = ((u[:, 0] * gu[:, 0] + u[:, 1] * gu[:, 1]) + u[:, 2] * gu[:, 2]).astype(F32)[:, None]
    return np.concatenate([go, gd + (gu - u * ug) / nrm], axis=1).astype(F32)


@pytest.mark.parametrize("B,N", [(1, 1), (17, 65), (255, 3)])
def test_rays_reduce_emulation_stays_inside_its_bound(oracle, B, N):
    rays, ts = S.crafted_rays(B, N, 100 + B)
    rng = np.random.Generator(np.random.PCG64(B))
    d_q = (rng.standard_normal((B * N, 6)) * np.array([1e3, 1e3, 1e3, 1, 1, 1])).astype(F32)
    want, bound = S.rays_reduce(rays, ts, d_q)
    got = _reduce_f32(rays, ts, d_q)
    worst = float(S.ratio(got, want, bound).max())
    print(f"CPU rays_reduce B={B} N={N}: worst ratio {worst:.4f}")
    assert worst <= 1
    # float64 autograd through the oracle's query_points says the same
    r64 = torch.from_numpy(rays).double().requires_grad_(True)
    q, _ = oracle.query_points(r64, torch.from_numpy(ts).double())
    (q * torch.from_numpy(d_q).double()).sum().backward()
    assert np.abs(r64.grad.numpy() - want).max() <= 1e-11 * np.abs(want).max()
    # a dropped sample, a missing projection: both outside
    assert S.ratio(_reduce_f32(rays, ts, d_q * (np.arange(B * N)[:, None] % N != N - 1)), want, bound).max() > 1
    noproj = got.copy()
    noproj[:, 3:] += ((rays[:, 3:] / np.linalg.norm(rays[:, 3:], axis=1, keepdims=True) ** 3)
                      * (rays[:, 3:] * d_q.reshape(B, N, 6)[:, :, 3:].sum(1)).sum(1, keepdims=True)).astype(F32)
    assert S.ratio(noproj, want, bound).max() > 1


# ---- why: the end-to-end rule on the inputs of test_nerf_forward_input_gradient -----------------------------------------
def _old_rule_inputs(kind):
    from nerf_simple_amd.utils import synthetic
    sd = synthetic.synthetic_state_dict(0, kind)
    P = 1000
    g = torch.Generator().manual_seed(0)
    xyz = torch.rand(P, 3, generator=g) * 2 - 1
    d = torch.randn(P, 3, generator=g)
    v = torch.cat([xyz, d / d.norm(dim=1, keepdim=True)], 1)          # test_gpu_input_gradients._points(P)
    G = torch.randn(P, 4, generator=torch.Generator().manual_seed(5))
    return sd, v, G


def test_the_end_to_end_rule_cannot_see_the_direction_columns(oracle):
    """On the inputs of tests/test_gpu_input_gradients.py::test_nerf_forward_input_gradient (structured weights, P = 1000)
    a gradient whose three direction columns are ZERO satisfies input_grad_model.bound_bf16 with room to spare, and so does
    one that keeps nothing but encoder levels 8 and 9 of the position; the per-element rule rejects the first on every point.
    Figures (float64): max |d v[:, :3]| 4562.8, max |d v[:, 3:]| 3.62, bound_bf16 0.375, rel_err of the zero-direction
    mutant 7.9e-4, of the levels-8-9-only mutant 0.358; on default weights 0.1375 against 0.1718."""
    sd, v, G = _old_rule_inputs("structured")
    g64, _ = IG.points_grad(IG.exact_forward, sd, v, G, torch.float64)
    g32, _ = IG.points_grad(IG.exact_forward, sd, v, G, torch.float32)
    g16, _ = IG.points_grad(IG.emulated_forward, sd, v, G, torch.float32)
    bound = IG.bound_bf16(g16, g32, g64)
    mutant = g64.clone()
    mutant[:, 3:] = 0
    err = IG.rel_err(mutant, g64)
    top_x, top_d = float(g64[:, :3].abs().max()), float(g64[:, 3:].abs().max())
    # the float64 gradient that keeps only levels 8 and 9 of the position: d posx from autograd on the encoder's output
    v64 = v.double()
    x, d = oracle.positional_encoder(v64)
    x.requires_grad_(True)
    orig = oracle.positional_encoder
    try:
        oracle.positional_encoder = lambda vec, Lp=10, Ld=4: (x, d)
        (oracle.nerf_forward({k: t.double() for k, t in sd.items()}, v64) * G.double()).sum().backward()
    finally:
        oracle.positional_encoder = orig
    coord, level, trig = S.columns(S.LP)
    a = v64.numpy()[:, coord] * 2.0 ** np.maximum(level, 0)
    J = np.where(level < 8, 0.0, np.where(trig == 0, 2.0 ** level * np.cos(a), -(2.0 ** level) * np.sin(a)))
    high = np.zeros((1000, 6))
    high[:, :3] = (J * x.grad.numpy()) @ (coord[:, None] == np.arange(3)[None, :])
    err_high = IG.rel_err(torch.from_numpy(high), g64)
    print(f"OLD RULE structured: max|dx| {top_x:.1f} max|dd| {top_d:.3f} bound_bf16 {bound:.4f} zero-direction {err:.3e} "
          f"levels 8-9 only {err_high:.4f}")
    assert top_x == pytest.approx(4562.8, rel=1e-3) and top_d == pytest.approx(3.62, rel=5e-3)
    assert bound == pytest.approx(0.375, rel=2e-2)
    assert err == pytest.approx(7.9e-4, rel=2e-2) and err <= bound
    assert err_high == pytest.approx(0.358, rel=2e-2) and err_high <= bound
    # the same mutant of the bf16 chain's own result, against the stage model of the chain's stored operands
    posx, posd = orig(v)
    posx64 = torch.cat([posx.bfloat16().float(), torch.full((1000, 1), 7.0)], dim=1)
    posd32 = torch.cat([posd.bfloat16().float(), torch.full((1000, 5), 7.0)], dim=1)
    bufs = C.emulate_chain(sd, posx64, posd32, G)
    dY0, dY5, dY9 = bufs["dY"][0], bufs["dY"][5], bufs["dY"][9][:, :128]
    params = S.flat_params(sd)
    dys = S.craft_dys(dY0, dY5, dY9, 1000)
    pts = v.numpy()
    Wx, Wd = S.stored_weights(params)
    want, bnd = S.stage(dY0, dY5, dY9, Wx, Wd, pts)
    good = emulate(params, dys, pts, 1000)
    bad = emulate(params, dys, pts, 1000, "zero_direction")
    r_good, r_bad = S.ratio(good, want, bnd), S.ratio(bad, want, bnd)
    print(f"NEW RULE structured: correct emulation {r_good.max():.4f}; zero-direction mutant fails on "
          f"{int((r_bad[:, 3:] > 1).any(1).sum())} of 1000 points, worst ratio {r_bad.max():.3g}")
    assert r_good.max() <= 1
    assert IG.rel_err(torch.from_numpy(bad), g64) <= bound             # the old rule passes the mutant of the chain, too
    assert (r_bad[:, 3:] > 1).any(1).sum() >= 990 and r_bad.max() > 1e3


def test_the_end_to_end_rule_on_default_weights():
    sd, v, G = _old_rule_inputs("default")
    g64, _ = IG.points_grad(IG.exact_forward, sd, v, G, torch.float64)
    g32, _ = IG.points_grad(IG.exact_forward, sd, v, G, torch.float32)
    g16, _ = IG.points_grad(IG.emulated_forward, sd, v, G, torch.float32)
    bound = IG.bound_bf16(g16, g32, g64)
    mutant = g64.clone()
    mutant[:, 3:] = 0
    err = IG.rel_err(mutant, g64)
    print(f"OLD RULE default: bound_bf16 {bound:.4f} zero-direction {err:.4f}")
    assert bound == pytest.approx(0.1718, rel=2e-2) and err == pytest.approx(0.1375, rel=2e-2) and err <= bound
