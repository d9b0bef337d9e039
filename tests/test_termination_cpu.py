"""Early ray termination without a GPU: the library's host side (the symbol, its argtypes, argument checking -- no entry point
touches a device here), the numpy model (tests/termination_model.py) against itself and against the masked-render model, the
informativeness of the inputs tests/test_gpu_termination.py uses, and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import occupancy_model as M
import termination_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUP = -1, -2
NEW = ("nerf_amd_termination_advance", "nerf_amd_termination_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- the library without a GPU -----------------------------------------------------------------------------------------
def test_symbols_exported_bound_and_abi_unchanged(lib):
    from nerf_simple_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    for s in NEW:
        assert hasattr(raw, s) and s in _lib.EXPORTS, s
        assert re.search(r"\b" + s + r"\(", header), s
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    f = lib.nerf_amd_termination_advance
    assert f.restype is i32
    assert list(f.argtypes) == [vp, vp, vp, i64, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, i64, vp, vp, vp, i64, f32, i32, i32,
                                i32, i32, vp, vp, vp, vp, vp, i64, i32, vp]
    assert lib.nerf_amd_termination_workspace_bytes.restype is i64
    assert lib.nerf_amd_abi_version() == 5
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    for B in (0, 1, 2048, 2049, 640000):
        n = lib.nerf_amd_termination_workspace_bytes(B)
        assert n >= 12 * B and n % 256 == 0           # a carry and two counts per ray
    assert lib.nerf_amd_termination_workspace_bytes(-1) == EINVAL
    assert lib.nerf_amd_termination_workspace_bytes((1 << 32) + 1) == EUNSUP


def test_entry_point_refuses_bad_arguments_on_the_host(lib):
    """Every call below must return before anything is launched: the pointers are fake."""
    P, Q = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)      # non-null, 16-aligned, never dereferenced
    odd4, odd8 = ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1008)

    def adv(raw=P, ms=P, os_=P, rows=10, rays=P, u=P, tbins=P, flags=0, m0=P, o0=P, raw0=P, rows0=100, eps=0.1, S=32, s=(0, 32, 64),
            trans=P, mn=Q, on=Q, tot=P, ws=P, B=4, N=128):
        return lib.nerf_amd_termination_advance(raw, ms, os_, rows, rays, u, tbins, flags, 0, 0, m0, o0, raw0, rows0,
                                                ctypes.c_float(eps), S, *s, trans, mn, on, tot, ws, B, N, None)

    first = dict(raw=None, ms=None, os_=None, rows=0, s=(0, 0, 32))
    assert adv(rays=None) == EINVAL and adv(B=0) == 0 and adv(B=0, **first) == 0      # (the defaults themselves would be launched)
    einval = (dict(rays=None), dict(u=None), dict(tbins=None), dict(m0=None), dict(o0=None), dict(raw0=None), dict(trans=None),
              dict(mn=None), dict(on=None), dict(tot=None), dict(ws=None), dict(ms=None), dict(os_=None),
              dict(B=-1), dict(N=0), dict(N=-3), dict(rows=-1), dict(rows0=-1), dict(raw=None),      # rows without their tensor
              dict(flags=16), dict(flags=128), dict(flags=4), dict(flags=4 | 1), dict(flags=4 | 2, u=None), dict(flags=4 | 2, u=odd4),
              dict(flags=1, u=None, tbins=None),
              dict(raw=odd4), dict(raw=odd8), dict(raw0=odd8), dict(ms=odd4), dict(os_=odd4), dict(m0=odd4), dict(o0=odd4),
              dict(mn=odd4), dict(on=odd4), dict(tot=odd4), dict(ws=odd8), dict(trans=ctypes.c_void_p(0x1002)),
              dict(mn=P), dict(on=P),                                                               # the scan is not in place
              dict(eps=0.0), dict(eps=1.0), dict(eps=-0.5), dict(eps=1.5), dict(eps=float("nan")), dict(eps=float("inf")),
              dict(S=0), dict(S=8), dict(S=48), dict(S=128), dict(S=-32), dict(S=33),
              dict(s=(0, 32, 32)), dict(s=(0, 32, 96)), dict(s=(32, 0, 32)), dict(s=(0, 16, 48)), dict(s=(16, 48, 80)),
              dict(s=(0, 64, 96)), dict(s=(-32, 0, 32)), dict(s=(96, 128, 160)), dict(s=(0, 0, 0)), dict(s=(0, 0, 64)),
              dict(s=(64, 64, 96)), dict(s=(0, 0, 32)),                                              # raw_slab with nothing to retire
              dict(s=(96, 128, 128), N=100), dict(s=(96, 100, 128), N=100))
    for kw in einval:
        assert adv(**kw) == EINVAL, kw
    for kw in (dict(rows=5), dict(s=(0, 0, 64)), dict(s=(0, 0, 16)), dict(s=(32, 32, 64))):
        assert adv(**{**first, **kw}) == EINVAL, kw
    # N > 768, B > 2^32: unsupported, as the masked render has it; a bad eps or slab is a bad argument at any size
    for kw in (dict(N=769, s=(0, 32, 64)), dict(N=1024), dict(B=(1 << 32) + 1)):
        assert adv(**kw) == EUNSUP, kw
        assert adv(eps=2.0, **kw) == EINVAL and adv(S=17, **kw) == EINVAL, kw


# ---- the numpy model ---------------------------------------------------------------------------------------------------
def random_case(seed, B, N, p_live, opaque=0.1):
    rng = np.random.default_rng(seed)
    alpha = rng.random((B, N)) ** 4                                  # mostly thin ...
    alpha = np.where(rng.random((B, N)) < opaque, 0.7 + 0.3 * rng.random((B, N)), alpha)     # ... with opaque surfaces
    return alpha.astype(np.float32), rng.random((B, N)) < p_live


@pytest.mark.parametrize("S", T.SLABS)
def test_model_rule(S):
    for seed, (B, N, p) in enumerate(((40, 3, 0.9), (40, 33, 0.7), (60, 64, 1.0), (60, 65, 0.5), (80, 128, 0.6), (30, 192, 1.0))):
        alpha, live0 = random_case(seed, B, N, p)
        K = T.slab_count(N, S)
        assert len(T.advance_calls(N, S)) == K + 1 and T.advance_calls(N, S)[-1][1:] == (N, N)
        prev_eval = None
        for eps in (1e-30, 1e-4, 0.01, 0.1, 0.5, 0.99):
            Tk, ev, term = T.terminate(alpha, live0, S, eps)
            assert Tk.shape == (B, K) and (Tk[:, 0] == 1).all() and not term[:, 0].any()
            assert (np.diff(Tk, axis=1) <= 0).all(), "T never grows"
            assert (term[:, 1:] >= term[:, :-1]).all(), "termination is permanent: monotone in k"
            assert (ev <= live0).all()
            if eps < Tk.min():
                assert (ev == live0).all(), "M* = M0 when eps is below every T"
            if prev_eval is not None:
                assert (ev <= prev_eval).all(), "monotone in eps: a larger eps evaluates a subset"
            prev_eval = ev
            # M* is M0 & (the slab of sample i is not terminated)
            slab_of = np.arange(N) // S
            assert (ev == (live0 & ~term[:, slab_of])).all()
            # frozen after termination
            for k in range(1, K):
                assert (Tk[term[:, k - 1], k] == Tk[term[:, k - 1], k - 1]).all()
        full = T.terminate(alpha, live0, S, 1e-300)[0]                # nothing terminates: the un-terminated T
        assert full.min() > 1e-300 and (T.terminate(alpha, live0, S, full.min() / 2)[1] == live0).all()
        assert T.terminate(alpha, live0, S, 0.5)[1].sum() < live0.sum() or N <= S


@pytest.mark.parametrize("S", T.SLABS)
def test_a_nan_row_never_terminates_its_ray(S):
    alpha, live0 = random_case(7, 50, 128, 1.0, opaque=0.3)
    alpha[:, 5] = np.nan                                             # a NaN row in the first slab of every ray
    for eps in (0.01, 0.5, 0.99):
        Tk, ev, term = T.terminate(alpha, live0, S, eps)
        assert np.isnan(Tk[:, 1:]).all() and not term.any() and (ev == live0).all()
    clean, _ = random_case(7, 50, 128, 1.0, opaque=0.3)
    assert T.terminate(clean, live0, S, 0.5)[2].any()                # the same rays without the NaN do terminate


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("grid,eps", [("all", 0.01), ("all", 0.1), ("ball", 0.1), ("ball", 0.5), ("all", 0.5)])
def test_model_composite_is_the_masked_composite_under_the_evaluated_mask_and_stays_in_bound(oracle, synthetic, dtype, grid, eps):
    N, S = 128, 32
    _, rays, u, ts, q, dn = T.view(oracle, synthetic, N)
    raw = T.view_raw(oracle, synthetic, "structured", N).to(dtype)
    ts, dn = ts.to(dtype), dn.to(dtype)
    live0 = T.view_live(oracle, synthetic, grid, N)
    (rgb_t, depth_t, acc_t, alpha_t, w_t), Tk, ev = T.terminated_composite(raw, ts, dn, live0, S, eps)
    assert ev.sum() < live0.sum(), "the case must drop something"
    # the vectorised rule sees the same mask from the same alphas
    Tk2, ev2, term2 = T.terminate(T.alphas(raw, ts, dn).numpy(), live0, S, eps)
    if dtype == torch.float32:
        assert (ev2 == ev).all() and np.allclose(Tk2, Tk.numpy().astype(np.float64), rtol=1e-6, atol=0)
    rgb, disp, alpha, acc, w = T.masked_composite(oracle, raw, ts, dn, ev)
    assert float((alpha - alpha_t).abs().max()) == 0.0 and float((w - w_t).abs().max()) == 0.0
    tiny = torch.finfo(dtype).eps
    assert float((rgb - rgb_t).abs().max()) <= 64 * tiny * max(1.0, float(rgb_t.abs().max()))
    assert float((acc - acc_t).abs().max()) <= 64 * tiny
    dropped = torch.from_numpy(live0 & ~ev)
    assert (alpha[dropped] == 0).all() and (w[dropped] == 0).all()
    # against the un-terminated masked render: |d rgb| < eps max|c| over the dropped samples, |d acc| < eps
    rgb0, _, _, acc0, _ = M.masked_composite(oracle, raw, ts, dn, live0)
    brgb, bacc = T.bounds(raw, ev, live0, eps)
    slack = 4 * N * tiny
    assert ((rgb - rgb0).abs().amax(1) <= brgb + slack * raw[..., :3].abs().amax()).all()
    assert ((acc - acc0).abs() <= bacc + slack).all()
    assert float((acc - acc0).abs().max()) > 0, "termination changed nothing"
    never = torch.from_numpy(~(live0 & ~ev).any(1))
    assert (rgb[never] == rgb0[never]).all() and (acc[never] == acc0[never]).all(), "a ray that drops nothing is what it was"


# ---- the GPU tests' inputs are informative (recomputed on the CPU oracle) -------------------------------------------------
@pytest.mark.parametrize("kind,grid,eps,lo,hi", [("structured", "all", 0.1, 0.1, 0.9), ("structured", "ball", 0.5, 0.1, 0.9),
                                                 ("default", "all", 1e-4, 0.0, 0.0), ("default", "ball", 1e-4, 0.0, 0.0)])
def test_gpu_inputs_are_informative(oracle, synthetic, kind, grid, eps, lo, hi):
    N, S = 128, 32
    _, rays, u, ts, q, dn = T.view(oracle, synthetic, N)
    assert rays.shape[0] == 400
    raw = T.view_raw(oracle, synthetic, kind, N)
    live0 = T.view_live(oracle, synthetic, grid, N)
    Tk, ev, term = T.terminate(T.alphas(raw, ts, dn).numpy(), live0, S, eps)
    share = T.terminated_share(term)
    print(f"{kind} {grid} eps={eps}: terminated share {share:.4f}, dropped {1 - ev.sum() / live0.sum():.4f} of the live samples")
    assert lo <= share <= hi
    if hi == 0.0:
        assert (ev == live0).all()


# ---- refusals that need no device --------------------------------------------------------------------------------------
def test_bad_eps_or_slab_and_a_foreign_terminate_raise():
    from nerf_simple_amd.utils import nets, occupancy, rendering
    ok = occupancy.EarlyTermination(0.01, 32)
    assert ok.slab == 32 and ok.eps == float(np.float32(0.01)) and ok.last_stats is None
    for S in (16, 32, 64, np.int64(16)):
        assert occupancy.EarlyTermination(1e-3, S).slab == int(S)
    for eps in (0, 0.0, 1, 1.0, -0.1, 2, float("nan"), float("inf"), 1e-60, 1 - 1e-12, "small", None):
        with pytest.raises(ValueError, match="eps"):
            occupancy.EarlyTermination(eps, 32)
    for S in (0, 8, 48, 128, 32.0, "32", None, True):
        with pytest.raises(ValueError, match="slab"):
            occupancy.EarlyTermination(0.01, S)
    with pytest.raises(TypeError):
        occupancy.EarlyTermination()                                 # no defaults
    with pytest.raises(TypeError):
        occupancy.EarlyTermination(0.01)
    net = nets.Nerf()                       # (its nn.Linear initialisers draw from the CPU generator)
    state = torch.get_rng_state()
    for bad in (0.01, "term", (0.01, 32)):
        with pytest.raises(TypeError, match="EarlyTermination"):
            occupancy.check_terminable(bad, None, net, False)
    with pytest.raises(RuntimeError, match="inference only"):
        occupancy.check_terminable(ok, None, net, False)             # grad mode, a trainable net
    with torch.no_grad():
        occupancy.check_terminable(ok, None, net, False)
        with pytest.raises(RuntimeError, match="default Nerf"):
            occupancy.check_terminable(ok, None, object(), False)
        with pytest.raises(TypeError, match="OccupancyGrid"):
            occupancy.check_terminable(ok, "grid", net, False)
        with pytest.raises(RuntimeError):
            rendering.render_nerf(torch.zeros(2, 6), net, 8, terminate=ok)      # CPU rays: the usual error
    assert torch.equal(torch.get_rng_state(), state), "a refused call must not consume the CPU generator"
