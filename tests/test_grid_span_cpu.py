"""The grid span without a GPU (csrc/grid_span.hip, utils/box.py ``GridSpan``): the export and prototype
of nerf_amd_span_positions, its argument rules call by call (tests/golden/abi_refusals_span.json, written from the rules in
include/nerf_amd.h: every call is refused or is an empty problem, so nothing is launched), ``GridSpan`` as a validated frozen
value, ``box=`` accepting it, the refusals -- before any launch and any RNG draw -- and the properties of the model
(tests/grid_span_model.py): conservative, equal to the grid's box when every cell is live, and what it buys on the ball."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import box_model as BM
import grid_span_model as M
import test_gpu_occupancy_graphed as OG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_refusals_span.json")
FAKE = 0x1000
NEW = "nerf_amd_span_positions"
TN, TF = BM.TN, BM.TF

with open(FIXTURE) as _f:
    CASES = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _arg(a):
    """"P": an aligned fake address; "P1" ...: the same address off by that many bytes; "nan" / "inf" / "-inf": the float; a
    list: a HOST float[3]"""
    if isinstance(a, list):
        return (ctypes.c_float * 3)(*[float(x) for x in a])
    if isinstance(a, str) and a.startswith("P"):
        return FAKE + int(a[1:] or 0)
    return float(a) if isinstance(a, str) else a


# ---- the library -------------------------------------------------------------------------------------------------------------
def test_export_header_and_ctypes_agree(lib):
    from nerf_simple_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    assert lib.nerf_amd_abi_version() == 5 and "#define NERF_AMD_ABI_VERSION 5" in header      # purely additive
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert NEW in _lib.EXPORTS and hasattr(raw, NEW) and len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    protos = re.findall(r"^int " + NEW + r"\(([^;]*)\);", header, re.M)
    assert len(protos) == 1
    params = [p.strip() for p in protos[0].replace("\n", " ").split(",")]
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["rays", "u", "tbins01", "flags", "seed", "ray_id0", "bits", "nx", "ny", "nz", "h_lo", "h_hi", "h_inv_step",
                     "probes", "tn", "tf", "ts", "span", "hit", "B", "N", "stream"]
    res, args = _lib._SIGNATURES[NEW]
    assert res is ctypes.c_int and len(args) == len(params)
    for p, a in zip(params, args):
        want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float ") else
                ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_uint64 if p.startswith("uint64_t") else
                ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
        assert a is want, (p, a)
    assert "int32_t* hit" in protos[0] and "const uint32_t* bits" in protos[0]
    # the header states the definition under its heading
    comment = header[header.index("grid span"):header.index("int " + NEW)]
    for phrase in ("e_0 = a, e_K = b exactly", "CLAMPED into [0, C - 1]", "CONSERVATIVE", "probes >= 2 max(C_a)", "8 cells"):
        assert phrase in comment, phrase
    csrc = os.path.join(ROOT, "nerf-simple_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "grid_span.hip" in make and "grid_span_device.h" in make
    kernel = open(os.path.join(csrc, "grid_span.hip")).read()
    # the jitter rule, the slab routine and the placement are reused, not restated
    assert "fetch_point_rays<false>(" in kernel and "box_place(" in kernel and kernel.count("__global__") == 1
    assert "atomicAdd" not in kernel and "__hip_atomic" not in kernel and "__shared__" not in kernel
    device = open(os.path.join(csrc, "grid_span_device.h")).read()
    assert '#include "ray_box_device.h"' in device and "ray_box_span(" in device and "BoxSpan ray_box_span(" not in device
    assert "__ballot(" in device and "__global__" not in device and "__fdiv_rn(" in device
    assert "nerf_amd_launch_span_positions(" in open(os.path.join(csrc, "launchers.h")).read()


def test_fixture_covers_every_rule():
    from nerf_simple_amd import _lib
    assert {c["fn"] for c in CASES} == {NEW}
    assert all(len(c["args"]) == len(_lib._SIGNATURES[NEW][1]) and c["expect"] in (0, -1, -2) for c in CASES)
    assert sum(c["note"].startswith("two rules:") for c in CASES) >= 6
    ints = {a for c in CASES for a in c["args"] if isinstance(a, int)}
    assert {768, 769, 1 << 32, (1 << 32) + 1, -1, 63, 65, 1024, 1088} <= ints
    assert {0, -1, -2} == {c["expect"] for c in CASES}
    for k in (10, 11, 12):                                                                        # lo, hi, inv_step
        assert any(c["args"][k] is None for c in CASES), k
        assert {"nan", "inf", "-inf"} <= {str(x) for c in CASES if isinstance(c["args"][k], list) for x in c["args"][k]}, k
    assert any(c["args"][6] is None for c in CASES)                                               # no bits
    assert {1} <= {c["args"][7] for c in CASES} and {1} <= {c["args"][8] for c in CASES} and {1} <= {c["args"][9] for c in CASES}
    probes = {c["args"][13] for c in CASES}
    assert {0, 32, 63, 64, 65, 128, 192, 256, 1024, 1088} <= probes
    for k in (0, 1, 2, 6, 16, 17, 18):                                                            # every buffer, misaligned
        assert any(str(c["args"][k]).startswith("P") and str(c["args"][k]) != "P" for c in CASES), k
    assert {0, 1, 2, 3, 4, 5, 6, 7, 64} <= {c["args"][3] for c in CASES}                          # every jitter mode and a bad bit


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"span_positions-{i}")
def test_abi_refusal(lib, i):
    case = CASES[i]
    assert getattr(lib, case["fn"])(*[_arg(a) for a in case["args"]]) == case["expect"], (case["note"], case["args"])


# ---- GridSpan ----------------------------------------------------------------------------------------------------------------
def fake_grid(R, outside="empty", bounds=M.BALL_BOUNDS):
    """An OccupancyGrid without a device: what GridSpan's validation looks at."""
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    g = OccupancyGrid.__new__(OccupancyGrid)
    g.words, g.resolution, g.bounds, g.outside = torch.zeros(1, dtype=torch.int32), tuple(R), bounds, outside
    return g


def test_grid_span_is_a_validated_frozen_value():
    from nerf_simple_amd.utils.box import GridSpan
    g = fake_grid((129, 129, 129))
    s = GridSpan(g)
    assert s.occupancy is g and s.probes == 256                        # the grid itself, not a copy
    assert GridSpan(fake_grid((9, 5, 7))).probes == 64 and GridSpan(fake_grid((33, 33, 33))).probes == 64
    assert GridSpan(fake_grid((34, 33, 33))).probes == 128 and GridSpan(fake_grid((513, 2, 2))).probes == 1024
    assert GridSpan(g, 512).probes == 512 and GridSpan(g, probes=1024).probes == 1024
    assert s == GridSpan(g, 256) and hash(s) == hash(GridSpan(g, 256)) and s != GridSpan(g, 512)
    assert s != GridSpan(fake_grid((129, 129, 129)))                   # another grid object is another span
    with pytest.raises(AttributeError, match="frozen"):
        s.probes = 512
    with pytest.raises(AttributeError, match="frozen"):
        del s.occupancy
    for bad in (0, 64, 192, 255, 257, 300, 1088, 2048, -256, 256.5, True, "256"):
        with pytest.raises((ValueError, TypeError)):
            GridSpan(g, bad)
    with pytest.raises(ValueError, match="outside='empty'"):
        GridSpan(fake_grid((129, 129, 129), outside="live"))
    with pytest.raises(ValueError, match="512 cells"):
        GridSpan(fake_grid((514, 9, 9)))
    with pytest.raises(TypeError, match="OccupancyGrid"):
        GridSpan(object())
    assert "probes=256" in repr(s)
    sig = inspect.signature(GridSpan.positions).parameters
    from nerf_simple_amd.utils.box import SceneBox
    assert list(sig) == list(inspect.signature(SceneBox.positions).parameters)
    for name in sig:
        assert (sig[name].kind, sig[name].default) == (inspect.signature(SceneBox.positions).parameters[name].kind,
                                                       inspect.signature(SceneBox.positions).parameters[name].default), name
    assert "no gradient" in GridSpan.positions.__doc__


def test_box_accepts_a_grid_span_and_refusals_come_before_any_draw():
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils import rendering as R
    from nerf_simple_amd.utils.box import GridSpan, check_box
    s = GridSpan(fake_grid((129, 129, 129)))
    assert check_box(s) is s and check_box(None) is None
    rays, gt = torch.zeros(2, 6), torch.zeros(2, 3)
    state = torch.get_rng_state()
    refused = (
        lambda: R.render_hierarchical(rays, None, None, box=s),
        lambda: R.render_hierarchical_view(None, None, None, None, box=s),
        lambda: T.train_step_hierarchical(None, None, None, rays, gt, box=s),
        lambda: R.render_guided(rays, None, 8, 8, None, box=s),
        lambda: R.render_guided_view(None, None, None, 8, 8, None, box=s),
        lambda: T.train_step_guided(None, None, rays, gt, 8, 8, None, box=s),
        lambda: T.GraphedCameraTrainStep(None, None, 2, 8, None, box=s),
        lambda: T.GraphedAppearanceTrainStep(None, None, 2, 8, None, rays_from=None, box=s),
        lambda: R.render_rays_sharded(None, rays, 2, box=s),
    )
    for call in refused:                                               # the exact message the scene box's refusals carry
        with pytest.raises(RuntimeError, match="box= serves the single-network renders and steps"):
            call()
    for call in (lambda: R.render_nerf(rays, None, 8, box=s, ts=torch.zeros(2, 8)),
                 lambda: T.render_nerf_masked(rays, None, 8, None, box=s, ts=torch.zeros(2, 8))):
        with pytest.raises(ValueError, match="not together with ts="):
            call()
    # neither a SceneBox nor a GridSpan: the TypeError names both
    for call in (lambda: R.render_nerf(rays, None, 8, box=object()), lambda: R.render_view(None, None, None, box="grid"),
                 lambda: T.render_nerf_masked(rays, None, 8, None, box=fake_grid((9, 9, 9))),
                 lambda: T.train_step(None, None, rays, gt, 8, box=()),
                 lambda: T.GraphedBoxTrainStep(None, None, 2, 8, None), lambda: T.GraphedMaskedBoxTrainStep(None, None, 2, 8, 3, None, 4)):
        with pytest.raises(TypeError, match="SceneBox.*GridSpan"):
            call()
    # what the placement would refuse, raised by the Python side before a draw; CPU rays: this package has no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        s.positions(rays, 8)
    with pytest.raises(RuntimeError, match="1 <= N <= 768"):
        T.GraphedBoxTrainStep(None, None, 2, 769, s)
    with pytest.raises(ValueError, match="tn < tf"):
        T.GraphedMaskedBoxTrainStep(None, None, 2, 8, s, None, 4, tn=6, tf=6)
    assert torch.equal(torch.get_rng_state(), state)


# ---- the model ---------------------------------------------------------------------------------------------------------------
def table_rays(oracle, synthetic):
    """The rays of the GPU tests: the scene box's case table (both sizes) and a subset of the 10,000 full rays."""
    full = OG.full_rays(oracle, synthetic)
    return torch.cat([BM.case_table(576)[0], BM.case_table(37)[0], full[torch.from_numpy(OG.subset(1000))]]).contiguous()


GRIDS = {"ball": (M.ball, 256), "hand_made": (M.hand_made, 64), "ball33": (M.ball33, 192)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", list(GRIDS) + ["ball-128", "ball-512"])
def test_span_is_conservative(oracle, synthetic, name, dtype):
    """4001 positions across [tn, tf] on every ray of the tables: one that the mark calls live (fp32, as the mark kernel forms
    it) lies within one segment length of [t0, t1], in the fp32 model and in the float64 one, and a ray with hit = 0 has none.
    (Measured here: the allowance is not used -- ``worst`` stays <= 0.)"""
    make, K = GRIDS[name.split("-")[0]]
    K = int(name.split("-")[1]) if "-" in name else K
    grid = make()
    rays = table_rays(oracle, synthetic)
    gap = torch.tensor([M.gap_ray()], dtype=torch.float32)
    rays = torch.cat([rays, gap]) if name == "hand_made" else rays
    t0, t1, hit, (a, b, _) = (x.float() if torch.is_tensor(x) and x.dtype == torch.float64 else x
                              for x in M.span(rays.to(dtype), grid, K, TN, TF))
    a, b = a.float(), b.float()
    t = np.linspace(TN, TF, 4001, dtype=np.float32)
    live = M.live_positions(rays, np.broadcast_to(t, (rays.shape[0], t.size)), grid)
    assert 0 < int(hit.sum()) < rays.shape[0] and bool(live.any())
    assert not live[~hit.numpy()].any(), int(live[~hit.numpy()].any(axis=1).sum())
    seg = ((b - a) / K).numpy()[:, None]
    out = np.maximum(t0.numpy()[:, None] - t[None, :], t[None, :] - t1.numpy()[:, None])           # > 0: outside [t0, t1]
    worst = float((out / seg)[live].max())
    print(f"{name}: {int(hit.sum())} of {rays.shape[0]} rays hit; farthest live position {worst:.3f} segment lengths outside")
    assert worst <= 1.0
    if name == "hand_made":                                             # the two cells and the gap between them: one interval
        assert float(t0[-1]) == 3.0 + 10 * 3.0 / 64 and float(t1[-1]) == 6.0 and bool(hit[-1])
        assert live[-1][(t > 3.5) & (t < 4.0)].all() and not live[-1][(t > 4.01) & (t < 5.49)].any()


@pytest.mark.parametrize("R", [(9, 5, 7), (33, 33, 33)])
def test_all_live_grid_is_the_grids_box(oracle, synthetic, R):
    bounds = M.HAND_BOUNDS if R == (9, 5, 7) else M.BALL_BOUNDS
    grid, rays, N = M.all_live(R, bounds), table_rays(oracle, synthetic), 65
    c = BM.unit_positions(torch.rand(rays.shape[0], N, generator=torch.Generator().manual_seed(1)), N)
    lo, hi = [float(x) for x in grid.lo], [float(x) for x in grid.hi]
    for K in (grid.least_probes(), 192, 1024):
        got, want = M.positions(rays, grid, K, TN, TF, c), BM.positions(rays, lo, hi, TN, TF, c)
        assert all(OG.same(g, w) for g, w in zip(got, want)), (R, K)
    dead = M.positions(rays, M.all_dead(R, bounds), 64, TN, TF, c)
    assert not bool(dead[2].any()) and bool((dead[1] == torch.tensor([TN, TF])).all())


def test_what_the_span_buys_on_the_ball(oracle, synthetic):
    """Live samples under three placements, N = 64, K = 256, the 10,000 full rays: span > live cells' box > plain, and the
    span's rays are at least 0.9 N live."""
    from nerf_simple_amd.utils import box as box_mod
    N, K, grid = 64, 256, M.ball()
    rays = OG.full_rays(oracle, synthetic)
    c = BM.unit_positions(OG.full_u(N), N)
    tight = box_mod._live_bounds(torch.from_numpy(grid.cells), grid.lo, grid.step, grid.bounds, 1)
    tight = [[float(np.float32(x)) for x in side] for side in tight]
    plain = BM.place(torch.full((rays.shape[0],), TN), torch.full((rays.shape[0],), TF), c)
    boxed, _, box_hit = BM.positions(rays, tight[0], tight[1], TN, TF, c)
    spanned, _, hit = M.positions(rays, grid, K, TN, TF, c)
    counts = {k: M.live_positions(rays, v, grid).sum(axis=1) for k, v in (("plain", plain), ("box", boxed), ("span", spanned))}
    hits = int(hit.sum())
    per_hit = {k: float(v[hit.numpy().astype(bool)].sum()) / hits for k, v in counts.items()}
    share = {k: float(v.sum()) / (rays.shape[0] * N) for k, v in counts.items()}
    print(f"{hits} of {rays.shape[0]} rays hit; live samples per hit ray {per_hit}; share of all samples live {share}")
    assert counts["span"].sum() > counts["box"].sum() > counts["plain"].sum()
    assert per_hit["span"] >= 0.9 * N
    assert not counts["span"][~hit.numpy().astype(bool)].any() and not counts["plain"][~hit.numpy().astype(bool)].any()
    assert 0.35 < hits / rays.shape[0] < 0.5


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 130])
def test_model_invariants(oracle, synthetic, N):
    rays = table_rays(oracle, synthetic)
    B = rays.shape[0]
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(N))
    c = BM.unit_positions(u, N)
    for name, (make, K) in GRIDS.items():
        ts, span, hit = M.positions(rays, make(), K, TN, TF, c)
        assert ts.dtype == torch.float32 and not torch.isnan(ts).any() and not torch.isnan(span).any(), name
        assert bool(((ts >= span[:, :1]) & (ts <= span[:, 1:])).all()) and bool((ts[:, 1:] >= ts[:, :-1]).all()), name
        miss = hit == 0
        assert bool(miss.any()) and not bool(miss.all()), name
        assert bool((span[miss] == torch.tensor([TN, TF])).all()), name
        assert bool(((span[~miss, 0] >= TN) & (span[~miss, 0] < span[~miss, 1]) & (span[~miss, 1] <= TF)).all()), name
        # float64: the same formula keeps the same invariants.  (No distance between the two is asserted: the 8 cells are a
        # superset of the cells a segment crosses, so a rounding at a cell face can switch a segment that owes its verdict to
        # a cell the ray never enters, and the next live one may be several segments on.  Both stay conservative:
        # test_span_is_conservative runs in either precision.)
        t0, t1, hit64, _ = M.span(rays.double(), make(), K, TN, TF)
        assert t0.dtype == torch.float64 and 0 < int(hit64.sum()) < B, name
        assert bool(((t0 >= TN) & (t0 < t1) & (t1 <= TF))[hit64].all()) and bool(((t0 == TN) & (t1 == TF))[~hit64].all()), name
