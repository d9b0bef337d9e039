"""The masked hierarchical pair without a GPU: the library's host side (the one new export, the ABI, the argument checking
of nerf_amd_volume_render_masked_mse_backward_pdf -- nothing touches a device), the composition model
(tests/occupancy_hierarchical_model.py) against its parts, the coarse live counts of the GPU tests' inputs
(tests/test_gpu_occupancy_hierarchical.py) from the existing CPU model, the Python surface and its refusals, and the
static ISA checks of the masked coarse head (csrc/occupancy_train.hip)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import occupancy_graphed_model as G
import occupancy_hierarchical_model as H
import occupancy_model as M
import occupancy_train_model as T

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R129 = (129, 129, 129)
NEW = "nerf_amd_volume_render_masked_mse_backward_pdf"
EINVAL, EUNSUP = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- the library without a GPU -----------------------------------------------------------------------------------------
def test_new_symbol_exported_bound_and_abi_unchanged(lib):
    from nerf_simple_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    assert hasattr(raw, NEW) and NEW in _lib.EXPORTS
    assert re.search(r"\b" + NEW + r"\(", header)
    f = getattr(lib, NEW)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert f.restype is i32
    assert list(f.argtypes) == [vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, i64, vp, vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp]
    assert lib.nerf_amd_abi_version() == 5
    # one added symbol: everything the library exported before is still there
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) and _lib.EXPORTS[-1] == NEW


def test_entry_point_refuses_bad_arguments_on_the_host(lib):
    """Every call below must return before anything is launched: the pointers are fake."""
    P = ctypes.c_void_p(0x1000)           # a non-null, 16-aligned address that is never dereferenced
    odd2, odd4, odd8 = ctypes.c_void_p(0x1002), ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1008)

    def head(raw=P, rays=P, u=P, tbins=P, flags=0, mask=P, offs=P, gt=P, u_f=P, rgb=P, d=P, ts_out=P, C=8, B=4, Nc=64, Nf=128):
        return getattr(lib, NEW)(raw, rays, u, tbins, flags, 0, 0, mask, offs, gt, u_f, rgb, d, ts_out, C, B, Nc, Nf, None)

    assert head(B=4, C=8, rays=None) == EINVAL                       # (sanity: the defaults themselves would be launched)
    einval = (dict(rays=None), dict(u=None), dict(tbins=None), dict(mask=None), dict(offs=None), dict(B=-1), dict(B=0), dict(Nc=0),
              dict(Nc=-3), dict(Nf=-1), dict(C=0), dict(C=-5), dict(C=4 * 64 + 1), dict(flags=16), dict(flags=128), dict(flags=4),
              dict(flags=4 | 1), dict(flags=4 | 2, u=None), dict(flags=4 | 2, u=odd4), dict(mask=odd4), dict(offs=odd4),
              dict(flags=1, u=None, tbins=None), dict(flags=1 | 2, u=None, tbins=None),       # given positions need their tensor
              dict(raw=None), dict(gt=None), dict(rgb=None), dict(d=None), dict(ts_out=None), dict(raw=odd4), dict(raw=odd8),
              dict(d=odd4), dict(d=odd8), dict(ts_out=odd2), dict(u_f=odd2), dict(gt=odd2), dict(rgb=odd2),
              dict(u_f=None),                                                                  # no u_f without the counter RNG
              dict(flags=1, u_f=None))
    for kw in einval:
        assert head(**kw) == EINVAL, kw
    # the sampler's limits: 3 <= Nc <= 256, Nc + Nf <= 512
    for kw in (dict(Nc=2), dict(Nc=1), dict(Nc=257, Nf=1), dict(Nc=300, Nf=0), dict(Nc=256, Nf=257), dict(Nc=64, Nf=449),
               dict(Nc=3, Nf=510)):
        assert head(**kw) == EUNSUP, kw
        assert head(C=0, **kw) == EINVAL, kw                           # a bad capacity is a bad argument at any size
    assert head(Nc=2, C=4 * 2 + 1) == EUNSUP                          # the size is judged before the capacity's upper end


# ---- the composition model ---------------------------------------------------------------------------------------------
def test_model_head_is_the_masked_chain_followed_by_the_oracle_sampler(oracle):
    """coarse_head = masked_outputs under mask_C -> MSE gradient by autograd -> oracle.sample_pdf on its w; the clamp only
    matters on an overflow, a dead sample has w = 0 exactly, and a ray with nothing kept gets the uniform rows."""
    rng = np.random.default_rng(11)
    gen = torch.Generator().manual_seed(5)
    for B, Nc, Nf, p in ((5, 3, 1, 0.6), (9, 64, 128, 0.2), (4, 66, 65, 0.3), (6, 8, 5, 0.0)):
        live = rng.random((B, Nc)) < p
        if p:
            live[0] = False                                            # one ray with nothing live
        total = int(live.sum())
        u_c = torch.rand(B, Nc, generator=gen)
        ts_c = oracle.sample_ts(u_c)
        dn = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=1)
        gt, u_f = torch.rand(B, 3, generator=gen), torch.rand(B, Nf, generator=gen)
        raw = torch.randn(total, 4, generator=gen, dtype=torch.float64)
        full = H.coarse_head(raw, ts_c.double(), dn.double(), live, max(total, 1), gt, u_f)
        for C in G.capacities(total, B, Nc):
            rgb, d, ts_f, w = H.coarse_head(raw, ts_c.double(), dn.double(), live, C, gt, u_f)
            kept = G.mask_C(live, C)
            assert d.shape == (C, 4) and (d[int(kept.sum()):] == 0).all()
            assert (w[torch.from_numpy(~kept)] == 0).all()
            assert ts_f.shape == (B, Nc + Nf) and (ts_f[:, 1:] >= ts_f[:, :-1]).all()
            none = torch.from_numpy(kept.sum(1) == 0)
            assert (rgb[none] == 0).all()
            assert torch.equal(ts_f[none], H.uniform_rows(ts_c.double(), u_f.double())[none])
            if C >= total:
                assert torch.equal(rgb, full[0]) and torch.equal(ts_f, full[2]) and torch.equal(d[:total], full[1][:total])
    # uniform rows: the new samples are the affine image of u over the interior bins' span
    ts_c = oracle.sample_ts(torch.full((1, 8), 0.5))
    z = H.uniform_rows(ts_c, torch.tensor([[0.0, 0.3, 0.5]]))
    mids = 0.5 * (ts_c[:, 1:] + ts_c[:, :-1])
    want = mids[0, 0] + torch.tensor([0.0, 0.3, 0.5]) * (mids[0, -1] - mids[0, 0])
    new = torch.tensor([v for v in z[0].tolist() if v not in ts_c[0].tolist()])
    assert torch.allclose(new, want, atol=1e-5)


# coarse live counts of the step-level inputs: (B, Nc, Nf, outside) -> P'_c
LIVE_COUNTS = {(576, 64, 128, "empty"): 4843, (576, 66, 65, "live"): 16858, (37, 64, 128, "live"): 1115,
               (37, 66, 65, "empty"): 405}


@pytest.mark.parametrize("case", sorted(LIVE_COUNTS))
def test_step_level_inputs_are_informative(oracle, synthetic, case):
    B, Nc, Nf, outside = case
    rays, _, u_c, u_f = H.pair_inputs(oracle, synthetic, B, Nc, Nf)
    assert u_f.shape == (B, Nf)
    _, q, _ = T.geometry(rays, u=u_c)
    live = T.live_of(q, M.ball_cells(R129, BOUNDS, 1.0), R129, BOUNDS, outside)
    M.require_informative(live, Nc, outside)
    total = int(live.sum())
    assert total == LIVE_COUNTS[case]
    if outside == "empty":
        assert int((live.sum(1) == 0).sum()) > 0                      # rays with no live coarse sample: uniform fine samples
        half = -(-total // 2)
        assert half not in set(M.offsets(live).tolist())              # the halved capacity cuts inside a ray


def test_pair_model_fine_pass_sees_its_own_live_fraction(oracle, synthetic):
    """the fine samples gather where the coarse weights are: on the analytic scene the fine pass's live fraction is not the
    coarse pass's (what the fine capacity has to be sized for)"""
    B, Nc, Nf = 37, 64, 128
    rays, gt, u_c, u_f = H.pair_inputs(oracle, synthetic, B, Nc, Nf)
    cells = M.ball_cells(R129, BOUNDS, 1.0)

    def forward(sd, pts):
        return T.scene_raw(pts)
    lc, lf, live_c, live_f, ts_f = H.pair_losses(forward, None, None, rays, u_c, u_f, cells, R129, BOUNDS, "empty", gt, torch.float32)
    assert live_c.shape == (B, Nc) and live_f.shape == (B, Nc + Nf) and ts_f.shape == (B, Nc + Nf)
    assert int(live_c.sum()) == 393
    assert torch.isfinite(lc) and torch.isfinite(lf)
    print(f"live fraction coarse {live_c.mean():.3f}, fine {live_f.mean():.3f}")
    assert live_f.mean() > live_c.mean()


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_python_surface():
    from nerf_simple_amd import training
    from nerf_simple_amd.utils import rendering
    cls = training.GraphedMaskedHierarchicalTrainStep
    assert issubclass(cls, training.GraphedHierarchicalTrainStep) and issubclass(cls, training.GraphedTrainStep)
    sig = inspect.signature(cls.__init__)
    assert list(sig.parameters)[:9] == ["self", "net_c", "net_f", "optimizer", "n_rays", "Nc", "Nf", "occupancy", "capacity"]
    assert sig.parameters["capacity"].default is inspect.Parameter.empty          # no default, as `level` has none
    for name in ("tn", "tf", "group", "device_rng", "seed", "ray_id0", "check_every", "rays_from", "select_mode", "buckets", "storage"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert callable(cls.counts) and callable(cls.step)
    for f in (training.train_step_hierarchical, rendering.render_hierarchical, rendering.render_hierarchical_view):
        p = inspect.signature(f).parameters["occupancy"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, f.__name__
    assert inspect.signature(training.render_nerf_masked).parameters["return_ts"].default is False


def test_capacity_pair_is_parsed_before_anything_else_runs():
    from nerf_simple_amd.training import _capacity_points
    assert _capacity_points(7, 100, "c") == 7 and _capacity_points(0.25, 576 * 64, "c") == 576 * 16
    assert _capacity_points(1e-9, 100, "c") == 1 and _capacity_points(1.0, 100, "c") == 100
    for bad, exc in ((0, ValueError), (101, ValueError), (1.5, ValueError), (0.0, ValueError), ("half", TypeError), (True, TypeError),
                     (None, TypeError)):
        with pytest.raises(exc):
            _capacity_points(bad, 100, "c")


def test_refusals_that_need_no_gpu_leave_the_generator_untouched():
    """what train_step_hierarchical / render_hierarchical / the graphed class refuse before they look at a device tensor"""
    from nerf_simple_amd import training
    from nerf_simple_amd.utils import rendering
    from nerf_simple_amd.utils.nets import Nerf
    a, b = Nerf(precision="bf16"), Nerf(precision="bf16")
    fp16 = Nerf(precision="fp16")
    cls = training.GraphedMaskedHierarchicalTrainStep
    cases = [
        ("one module twice", ValueError, lambda: training.train_step_hierarchical(a, a, None, None, None, occupancy=object())),
        ("two precisions", ValueError, lambda: training.train_step_hierarchical(a, fp16, None, None, None, occupancy=object())),
        ("Nc = 2", ValueError, lambda: training.train_step_hierarchical(a, b, None, None, None, 2, 8, occupancy=object())),
        ("Nc + Nf > 512", ValueError, lambda: training.train_step_hierarchical(a, b, None, None, None, 256, 257, occupancy=object())),
        ("graphed: storage", ValueError, lambda: cls(a, b, None, 8, 64, 128, object(), (0.5, 0.5), storage="e4m3")),
        ("graphed: buckets", ValueError, lambda: cls(a, b, None, 8, 64, 128, object(), (0.5, 0.5), buckets=2)),
        ("graphed: one module twice", ValueError, lambda: cls(a, a, None, 8, 64, 128, object(), (0.5, 0.5))),
        ("graphed: Nc = 257", ValueError, lambda: cls(a, b, None, 8, 257, 1, object(), (0.5, 0.5))),
        ("graphed: no rays", ValueError, lambda: cls(a, b, None, 0, 64, 128, object(), (0.5, 0.5))),
        ("graphed: not a grid", TypeError, lambda: cls(a, b, None, 8, 64, 128, object(), (0.5, 0.5))),
        ("graphed: no capacity", TypeError, lambda: cls(a, b, None, 8, 64, 128, object())),
    ]
    for what, exc, call in cases:
        state = torch.get_rng_state()
        with pytest.raises(exc):
            call()
        assert torch.equal(torch.get_rng_state(), state), what
    assert "occupancy" in inspect.signature(rendering.render_hierarchical_sharded).parameters or \
        inspect.signature(rendering.render_hierarchical_sharded).parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD


def test_new_kernel_passes_the_static_isa_checks():
    """tools/check_vmcnt.py (tests/static_isa.py) on the masked coarse head, the sampler instantiations of the masked compositor
    backward in csrc/occupancy_train.hip: exactly the four keys-per-lane ones, no counted vmcnt wait is short, no wide store
    has its data registers overwritten by the next instruction, and no kernel uses an atomic."""
    import static_isa
    heads = static_isa.masked_backward_instantiations(static_isa.checked_kernels("occupancy_train.hip"))
    assert [h for h in heads if h[1] > 0] == [("MseHead", 1), ("MseHead", 2), ("MseHead", 4), ("MseHead", 8)], heads
