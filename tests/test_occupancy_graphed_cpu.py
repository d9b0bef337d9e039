"""The graphed masked training step without a GPU: the library's host side (exports, ABI, argument checking of the two new
entry points -- nothing touches a device), the capacity model (tests/occupancy_graphed_model.py) against its definition
spelled out as a loop, the inputs of the GPU tests (tests/test_gpu_occupancy_graphed.py) with the live counts DESIGN.md
section 14 quotes, the Python surface, and the static ISA checks of csrc/occupancy_graph.hip."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import occupancy_graphed_model as G
import occupancy_model as M
import occupancy_train_model as T

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R129 = (129, 129, 129)
NEW = ("nerf_amd_occupancy_points_capped", "nerf_amd_volume_render_masked_mse_backward")
EINVAL, EUNSUP = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def step_inputs(oracle, synthetic, B, N):
    """the rays, targets and jitter of tests/test_gpu_training.py::test_fused_training_vs_oracle at this shape"""
    gen = torch.Generator().manual_seed(B * 1000 + N)
    pose = torch.from_numpy(oracle.spherical_to_pose(4, -30, 0)).float()
    side = int(np.ceil(np.sqrt(B)))
    rays = oracle.camera_rays(pose, [side, side, synthetic.focal_from_fov(side)])[:B].contiguous()
    gt = torch.rand(B, 3, generator=gen)
    u = torch.rand(B, N, generator=gen)
    return rays, gt, u


# ---- the library without a GPU -----------------------------------------------------------------------------------------
def test_new_symbols_exported_bound_and_abi_unchanged(lib):
    from nerf_simple_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    for s in NEW:
        assert hasattr(raw, s) and s in _lib.EXPORTS and getattr(lib, s).argtypes is not None, s
        assert re.search(r"\b" + s + r"\(", header), s
    assert len(lib.nerf_amd_occupancy_points_capped.argtypes) == 14
    assert len(lib.nerf_amd_volume_render_masked_mse_backward.argtypes) == 16
    assert lib.nerf_amd_abi_version() == 5
    # the pad point of the header is the model's
    m = re.search(r"#define NERF_AMD_OCCUPANCY_PAD_POINT \{([^}]*)\}", header)
    assert m and tuple(float(x.strip().rstrip("f")) for x in m.group(1).split(",")) == G.PAD_POINT
    assert all(abs(x) <= 1.0 for x in G.PAD_POINT)                    # inside the network's input range


def test_entry_points_refuse_bad_arguments_on_the_host(lib):
    """Every call below must return before anything is launched: the pointers are fake."""
    P = ctypes.c_void_p(0x1000)           # a non-null, 16-aligned address that is never dereferenced
    odd4, odd8 = ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1008)

    def emit(rays=P, u=P, tbins=P, flags=0, mask=P, offs=P, pts=P, counts=P, C=8, B=4, N=64):
        return lib.nerf_amd_occupancy_points_capped(rays, u, tbins, flags, 0, 0, mask, offs, pts, counts, C, B, N, None)

    def head(raw=P, rays=P, u=P, tbins=P, flags=0, mask=P, offs=P, gt=P, rgb=P, d=P, C=8, B=4, N=64):
        return lib.nerf_amd_volume_render_masked_mse_backward(raw, rays, u, tbins, flags, 0, 0, mask, offs, gt, rgb, d, C, B, N, None)

    common = (dict(rays=None), dict(u=None), dict(tbins=None), dict(mask=None), dict(offs=None), dict(B=-1), dict(B=0), dict(N=0),
              dict(N=-3), dict(C=0), dict(C=-5), dict(C=4 * 64 + 1), dict(flags=16), dict(flags=128), dict(flags=4),
              dict(flags=4 | 1), dict(flags=4 | 2, u=None), dict(flags=4 | 2, u=odd4), dict(mask=odd4), dict(offs=odd4))
    for kw in common:
        assert emit(**kw) == EINVAL, kw
        assert head(**kw) == EINVAL, kw
    for kw in (dict(pts=None), dict(counts=None), dict(counts=odd4), dict(pts=ctypes.c_void_p(0x1002))):
        assert emit(**kw) == EINVAL, kw
    for kw in (dict(raw=None), dict(gt=None), dict(rgb=None), dict(d=None), dict(raw=odd4), dict(raw=odd8), dict(d=odd4), dict(d=odd8)):
        assert head(**kw) == EINVAL, kw
    for f in (emit, head):
        assert f(N=513) == EUNSUP and f(N=768) == EUNSUP and f(N=513, C=4 * 513) == EUNSUP
        assert f(N=513, C=0) == EINVAL                                  # a bad capacity is a bad argument at any N


# ---- the capacity model ------------------------------------------------------------------------------------------------
def test_mask_C_is_the_first_C_live_samples_in_ray_major_order():
    rng = np.random.default_rng(7)
    for B, N, p in ((1, 1, 0.5), (5, 3, 0.4), (9, 64, 0.2), (7, 65, 0.3), (4, 130, 0.05), (6, 8, 0.0), (3, 8, 1.0)):
        live = rng.random((B, N)) < p
        total = int(live.sum())
        for C in G.capacities(total, B, N):
            kept = G.mask_C(live, C)
            assert np.array_equal(kept, G.mask_C_loop(live, C)), (B, N, C)
            assert not (kept & ~live).any() and int(kept.sum()) == min(total, C) == G.counts(live, C)[1]
            assert np.array_equal(M.offsets(kept), G.offsets_C(live, C)), (B, N, C)
            if total <= C:
                assert np.array_equal(kept, live)
            else:
                # the dead tail: every dropped live sample comes after every kept one in ray-major order
                flat_k, flat_d = np.flatnonzero(kept.reshape(-1)), np.flatnonzero((live & ~kept).reshape(-1))
                assert flat_d.size == total - C and (flat_k.size == 0 or flat_k.max() < flat_d.min())
            pts = G.capped_points(rng.random((total, 6)).astype(np.float32), C)
            assert pts.shape == (C, 6) and (pts[min(total, C):] == np.asarray(G.PAD_POINT, np.float32)).all()


LIVE_COUNTS = {(576, 64, "empty"): 4843, (576, 64, "live"): 16334, (37, 65, "empty"): 396, (37, 65, "live"): 1129,
               (300, 3, "empty"): 128, (64, 1, "empty"): 7}


@pytest.mark.parametrize("case", sorted(LIVE_COUNTS))
def test_step_level_inputs_are_informative_and_cut_inside_a_ray(oracle, synthetic, case):
    B, N, outside = case
    rays, _, u = step_inputs(oracle, synthetic, B, N)
    _, q, _ = T.geometry(rays, u=u)
    live = T.live_of(q, M.ball_cells(R129, BOUNDS, 1.0), R129, BOUNDS, outside)
    M.require_informative(live, N, outside)
    total = int(live.sum())
    assert total == LIVE_COUNTS[case]
    if case == (576, 64, "empty"):
        assert abs(live.mean() - 0.131) < 5e-4 and int((live.sum(1) == 0).sum()) == 335
    half = -(-total // 2)
    off = M.offsets(live)
    if N >= 64 and outside == "empty":                                # the inputs the halved-capacity step test uses
        assert half not in set(off.tolist())                         # ceil(P' / 2) cuts inside a ray, not between two
    assert half in G.capacities(total, B, N) and total in G.capacities(total, B, N)


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_python_surface():
    from nerf_simple_amd import training
    cls = training.GraphedMaskedTrainStep
    assert issubclass(cls, training.GraphedTrainStep)
    sig = inspect.signature(cls.__init__)
    assert list(sig.parameters)[:7] == ["self", "net", "optimizer", "n_rays", "N", "occupancy", "capacity"]
    assert sig.parameters["capacity"].default is inspect.Parameter.empty          # no default, as `level` has none
    for name in ("tn", "tf", "group", "device_rng", "seed", "ray_id0", "check_every", "rays_from", "select_mode"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert callable(cls.counts) and callable(cls.step)


# capacity argument at n_rays * N = 100 -> points, or the exception: what BOTH spellings gave while GraphedMaskedTrainStep
# still carried its own copy of the rule (recorded there, before the copy went)
CAPACITY_CASES = [(7, 7), (1, 1), (100, 100), (0, ValueError), (-3, ValueError), (101, ValueError), (0.25, 25), (0.999, 100),
                  (1.0, 100), (1e-9, 1), (0.0, ValueError), (-0.5, ValueError), (1.5, ValueError), (2.0, ValueError),
                  (float("nan"), ValueError), (True, TypeError), (False, TypeError), (None, TypeError), ("half", TypeError),
                  ((1, 2), TypeError), (np.int64(7), 7), (np.float32(0.5), 50)]


def test_capacity_rule_is_capacity_points(monkeypatch):
    """GraphedMaskedTrainStep's capacity rule and training._capacity_points are one function: the constructor hands its
    argument to it with n_rays * N as the total, and every case raises or returns the same under both spellings.  No GPU: a
    grid on another device than the optimizer's vector stops the constructor right behind the capacity."""
    from nerf_simple_amd import training
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.utils.nets import Nerf
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    net = Nerf(precision="bf16")
    opt = object.__new__(FusedAdam)
    opt.net, opt.flat = net, torch.zeros(1)
    occ = object.__new__(OccupancyGrid)
    occ.words = torch.zeros(1, device="meta")
    real, seen = training._capacity_points, []

    def spy(capacity, total, what):
        seen.append((total, real(capacity, total, what)))
        return seen[-1][1]
    monkeypatch.setattr(training, "_capacity_points", spy)
    for capacity, want in CAPACITY_CASES:
        del seen[:]
        if isinstance(want, type):
            with pytest.raises(want):
                real(capacity, 100, "capacity")
            with pytest.raises(want):
                training.GraphedMaskedTrainStep(net, opt, 10, 10, occ, capacity)
        else:
            assert real(capacity, 100, "capacity") == want, capacity
            with pytest.raises(RuntimeError, match="lives on"):
                training.GraphedMaskedTrainStep(net, opt, 10, 10, occ, capacity)
            assert seen == [(100, want)], (capacity, seen)


def test_new_kernels_pass_the_static_isa_checks():
    """tools/check_vmcnt.py (tests/static_isa.py) on the two kernels of the step: no counted vmcnt wait is short, no wide store
    has its data registers overwritten by the next instruction, and no kernel uses an atomic (every row is written by exactly
    one lane).  occ_emit_capped_kernel is csrc/occupancy_graph.hip's only kernel; the fused head is the (MseHead, 0)
    instantiation of the masked compositor backward in csrc/occupancy_train.hip."""
    import static_isa
    kernels = static_isa.checked_kernels("occupancy_graph.hip")
    assert len(kernels) == 1 and all("occ_emit_capped_kernel" in k for k in kernels), list(kernels)
    heads = static_isa.masked_backward_instantiations(static_isa.checked_kernels("occupancy_train.hip"))
    assert heads.count(("MseHead", 0)) == 1, heads
