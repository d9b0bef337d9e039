"""The scene box without a GPU (csrc/ray_box.hip, utils/box.py): the export and prototype of
nerf_amd_box_positions, its argument rules call by call (tests/golden/abi_refusals_box.json, written from the rules in
include/nerf_amd.h: every call is refused or is an empty problem, so nothing is launched), ``SceneBox`` as a validated frozen
value, the live cells' box on hand-made masks, ``box=`` keyword-only and off by default wherever it exists, the refusals --
before any launch and any RNG draw -- and the properties of the model (tests/box_model.py) on the case table the GPU tests
reuse."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import box_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_refusals_box.json")
FAKE = 0x1000
NEW = "nerf_amd_box_positions"

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
    list: a HOST float[3] (the box)"""
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
    assert names == ["rays", "u", "tbins01", "flags", "seed", "ray_id0", "h_lo", "h_hi", "tn", "tf", "ts", "span", "hit", "B", "N",
                     "stream"]
    res, args = _lib._SIGNATURES[NEW]
    assert res is ctypes.c_int and len(args) == len(params)
    for p, a in zip(params, args):
        want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float ") else
                ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_uint64 if p.startswith("uint64_t") else
                ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
        assert a is want, (p, a)
    assert "int32_t* hit" in protos[0]
    # the header comment states the definition and the line of the reference it generalises
    comment = header[header.index("scene box"):header.index("int " + NEW)]
    assert "utils/rendering.py:24-30" in comment and "t0 < t1" in comment and "NERF_AMD_TS_GIVEN" in comment
    csrc = os.path.join(ROOT, "nerf-simple_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "ray_box.hip" in make and "ray_box_device.h" in make
    kernel = open(os.path.join(csrc, "ray_box.hip")).read()
    # the jitter rule is reused, not restated; the slab routine lives in the header a fused variant can include
    assert "fetch_point_rays<false>(" in kernel and "philox" not in kernel and "ray_box_span(" in kernel
    assert "atomicAdd" not in kernel and "__hip_atomic" not in kernel and kernel.count("__global__") == 1
    device = open(os.path.join(csrc, "ray_box_device.h")).read()
    assert "BoxSpan ray_box_span(" in device and "__fdiv_rn(" in device and "__global__" not in device
    assert "nerf_amd_launch_box_positions(" in open(os.path.join(csrc, "launchers.h")).read()


def test_fixture_covers_every_rule():
    from nerf_simple_amd import _lib
    assert {c["fn"] for c in CASES} == {NEW}
    assert all(len(c["args"]) == len(_lib._SIGNATURES[NEW][1]) and c["expect"] in (0, -1, -2) for c in CASES)
    assert sum(c["note"].startswith("two rules:") for c in CASES) >= 4
    ints = {a for c in CASES for a in c["args"] if isinstance(a, int)}
    assert {768, 769, 1 << 32, (1 << 32) + 1, -1} <= ints
    assert {0, -1, -2} == {c["expect"] for c in CASES}
    scalars = {str(a) for c in CASES for a in c["args"] if isinstance(a, str)} | \
              {str(x) for c in CASES for a in c["args"] if isinstance(a, list) for x in a}
    assert {"nan", "inf", "-inf"} <= scalars
    assert any(str(a).startswith("P") and str(a) != "P" for c in CASES for a in c["args"])          # a misaligned address
    assert any(c["args"][6] is None for c in CASES) and any(c["args"][7] is None for c in CASES)   # a missing lo, a missing hi
    flags = {c["args"][3] for c in CASES}
    assert {0, 1, 2, 4, 6, 7, 64} <= flags                                                       # every jitter mode and a bad bit


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"box_positions-{i}")
def test_abi_refusal(lib, i):
    case = CASES[i]
    assert getattr(lib, case["fn"])(*[_arg(a) for a in case["args"]]) == case["expect"], (case["note"], case["args"])


# ---- SceneBox ----------------------------------------------------------------------------------------------------------------
def test_scene_box_is_a_validated_frozen_value():
    from nerf_simple_amd.utils.box import SceneBox
    b = SceneBox((-1, -0.75, -1.25), [1, 0.5, 0.75])
    assert b.lo == (-1.0, -0.75, -1.25) and b.hi == (1.0, 0.5, 0.75)
    assert b == SceneBox(np.float32([-1, -0.75, -1.25]), torch.tensor([1, 0.5, 0.75])) and hash(b) == hash(SceneBox(b.lo, b.hi))
    assert SceneBox((0.1, 0, 0), (1, 1, 1)).lo[0] == float(np.float32(0.1))                # held as the kernel sees it
    with pytest.raises(AttributeError, match="frozen"):
        b.lo = (0, 0, 0)
    with pytest.raises(AttributeError, match="frozen"):
        del b.hi
    for lo, hi in (((0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1)), ((0, 0, 0), (1, 1, 0)), ((0, 0, 2), (1, 1, 1)),
                   ((float("nan"), 0, 0), (1, 1, 1)), ((0, 0, 0), (1, float("inf"), 1)), ((float("-inf"), 0, 0), (1, 1, 1)),
                   (3.0, (1, 1, 1)), ((0, 0, 0), (1e39, 1, 1))):
        with pytest.raises(ValueError):
            SceneBox(lo, hi)
    assert "SceneBox(lo=(-1.0, -0.75, -1.25)" in repr(b)

    class G:
        bounds = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
    assert SceneBox.from_grid(G()) == SceneBox((-1.5,) * 3, (1.5,) * 3)
    with pytest.raises(TypeError):
        SceneBox.from_grid(object())
    with pytest.raises(TypeError):
        SceneBox.from_occupancy(object())


def test_live_cells_box_on_hand_made_masks():
    from nerf_simple_amd.utils import box as box_mod
    from nerf_simple_amd.utils.mesh import grid_axes
    R = (9, 5, 7)                                                   # 8 x 4 x 6 cells
    bounds = ((-2.0, -1.0, -1.5), (2.0, 1.0, 1.5))                  # steps 0.5, 0.5, 0.5
    lo, step = grid_axes(R, bounds)
    cells = torch.zeros(8, 4, 6, dtype=torch.bool)
    with pytest.raises(ValueError, match="no live cell"):
        box_mod._live_bounds(cells, lo, step, bounds, 1)
    cells[3, 1, 2] = True                                           # one cell: [-0.5, 0] x [-0.5, 0] x [-0.5, 0]
    assert box_mod._live_bounds(cells, lo, step, bounds, 0) == ([-0.5, -0.5, -0.5], [0.0, 0.0, 0.0])
    assert box_mod._live_bounds(cells, lo, step, bounds, 1) == ([-1.0, -1.0, -1.0], [0.5, 0.5, 0.5])
    assert box_mod._live_bounds(cells, lo, step, bounds, 2) == ([-1.5, -1.0, -1.5], [1.0, 1.0, 1.0])      # clamped to the grid
    corner = torch.zeros(8, 4, 6, dtype=torch.bool)
    corner[7, 3, 0] = True                                          # a corner cell: the widened box stops at the bounds
    assert box_mod._live_bounds(corner, lo, step, bounds, 1) == ([1.0, 0.0, -1.5], [2.0, 1.0, -0.5])
    full = torch.ones(8, 4, 6, dtype=torch.bool)
    for margin in (0, 1, 5):
        assert box_mod._live_bounds(full, lo, step, bounds, margin) == (list(bounds[0]), list(bounds[1]))
    two = corner | cells                                            # the box spans both
    assert box_mod._live_bounds(two, lo, step, bounds, 0) == ([-0.5, -0.5, -1.5], [2.0, 1.0, 0.0])


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_box_is_keyword_only_and_off_by_default():
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils import metrics, rendering as R
    from nerf_simple_amd.utils.box import SceneBox
    for fn in (R.render_nerf, R.render_view, T.render_nerf_masked, T.train_step, R.render_hierarchical, R.render_hierarchical_view,
               R.render_guided, R.render_guided_view, T.train_step_hierarchical, T.train_step_guided):
        p = inspect.signature(fn).parameters["box"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(metrics.evaluate).parameters.values())
    sig = inspect.signature(SceneBox.positions).parameters
    assert list(sig)[:5] == ["self", "rays", "N", "tn", "tf"] and (sig["tn"].default, sig["tf"].default) == (2, 6)
    for name, default in (("u", None), ("ts", None), ("device_rng", False), ("seed", 0), ("ray_id0", 0), ("return_span", False)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name
    for cls, lead in ((T.GraphedBoxTrainStep, ["self", "net", "optimizer", "n_rays", "N", "box"]),
                      (T.GraphedMaskedBoxTrainStep, ["self", "net", "optimizer", "n_rays", "N", "box", "occupancy", "capacity"])):
        s = inspect.signature(cls.__init__).parameters
        assert list(s)[:len(lead)] == lead and all(s[n].default is inspect.Parameter.empty for n in lead[1:]), cls
    assert issubclass(T.GraphedBoxTrainStep, T.GraphedTrainStep) and issubclass(T.GraphedMaskedBoxTrainStep, T.GraphedMaskedTrainStep)
    assert T.GraphedMaskedBoxTrainStep.__mro__.index(T._BoxSteps) < T.GraphedMaskedBoxTrainStep.__mro__.index(T._MaskedSteps)
    # the existing steppers' signatures are what they were
    assert "box" not in inspect.signature(T.GraphedTrainStep.__init__).parameters
    assert "box" not in inspect.signature(T.GraphedMaskedTrainStep.__init__).parameters
    for fn in (SceneBox.positions, R.render_nerf, T.train_step):
        assert "no gradient" in fn.__doc__, fn


def test_refusals_come_before_any_draw():
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils import rendering as R
    from nerf_simple_amd.utils.box import SceneBox
    b = SceneBox(M.LO, M.HI)
    rays, gt = torch.zeros(2, 6), torch.zeros(2, 3)
    state = torch.get_rng_state()
    refused = (
        lambda: R.render_hierarchical(rays, None, None, box=b),
        lambda: R.render_hierarchical_view(None, None, None, None, box=b),
        lambda: T.train_step_hierarchical(None, None, None, rays, gt, box=b),
        lambda: R.render_guided(rays, None, 8, 8, None, box=b),
        lambda: R.render_guided_view(None, None, None, 8, 8, None, box=b),
        lambda: T.train_step_guided(None, None, rays, gt, 8, 8, None, box=b),
        lambda: T.GraphedCameraTrainStep(None, None, 2, 8, None, box=b),
        lambda: T.GraphedAppearanceTrainStep(None, None, 2, 8, None, rays_from=None, box=b),
        lambda: R.render_rays_sharded(None, rays, 2, box=b),
    )
    for call in refused:
        with pytest.raises(RuntimeError, match="box= serves the single-network renders and steps"):
            call()
    # box= with ts=: the box places the positions
    for call in (lambda: R.render_nerf(rays, None, 8, box=b, ts=torch.zeros(2, 8)),
                 lambda: T.render_nerf_masked(rays, None, 8, None, box=b, ts=torch.zeros(2, 8))):
        with pytest.raises(ValueError, match="not together with ts="):
            call()
    # not a SceneBox: TypeError, wherever the keyword exists
    for call in (lambda: R.render_nerf(rays, None, 8, box=(M.LO, M.HI)), lambda: R.render_view(None, None, None, box="unit"),
                 lambda: T.render_nerf_masked(rays, None, 8, None, box=1), lambda: T.train_step(None, None, rays, gt, 8, box=()),
                 lambda: R.render_guided(rays, None, 8, 8, None, box=1),
                 lambda: T.GraphedBoxTrainStep(None, None, 2, 8, None), lambda: T.GraphedMaskedBoxTrainStep(None, None, 2, 8, 3, None, 4)):
        with pytest.raises(TypeError, match="SceneBox"):
            call()
    # what the placement would refuse, raised by the Python side before a draw; CPU rays: this package has no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        b.positions(rays, 8)
    with pytest.raises(RuntimeError, match="1 <= N <= 768"):
        T.GraphedBoxTrainStep(None, None, 2, 769, b)
    with pytest.raises(ValueError, match="tn < tf"):
        T.GraphedBoxTrainStep(None, None, 2, 8, b, tn=6, tf=6)
    assert torch.equal(torch.get_rng_state(), state)


# ---- the model on the case table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [37, 576])
def test_case_table_holds_every_class(B):
    rays, names = M.case_table(B)
    assert rays.shape == (B, 6) and rays.dtype == torch.float32
    cls = M.classify(rays)
    assert set(cls) == set(M.CLASSES)
    for name in M.CLASSES:
        assert int(cls[name].sum()) >= 1, name
    for i, name in enumerate(names):                       # every built ray IS of the class it was built for
        assert name == "random" or bool(cls[name][i]), (i, name)
    # the three ways an interval is clipped, and a hit that [tn, tf] cuts on both sides
    _, _, hit = M.span(rays.double(), M.LO, M.HI, M.TN, M.TF)
    assert 0 < int(hit.sum()) < B


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 130])
def test_model_properties(N):
    B = 37
    rays, _ = M.case_table(B)
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(N))
    c = M.unit_positions(u, N)
    ts, span, hit = M.positions(rays, M.LO, M.HI, M.TN, M.TF, c)
    assert ts.dtype == torch.float32 and not torch.isnan(ts).any() and not torch.isnan(span).any()
    t0, t1 = span[:, :1], span[:, 1:]
    assert bool(((ts >= t0) & (ts <= t1)).all())
    assert bool((ts[:, 1:] >= ts[:, :-1]).all())                                       # ascending, as c is
    assert bool((c[:, 1:] >= c[:, :-1]).all())
    miss = hit == 0
    assert bool((span[miss] == torch.tensor([M.TN, M.TF])).all())
    assert bool(((span[~miss, 0] >= M.TN) & (span[~miss, 1] <= M.TF) & (span[~miss, 0] < span[~miss, 1])).all())
    # a miss is the reference's own placement on [tn, tf], to the roundings of the two formulas
    ref = torch.linspace(M.TN, M.TF, N + 1)
    ts_ref = (ref[1] - ref[0]) * u + ref[:N]
    assert float((ts[miss] - ts_ref[miss]).abs().max()) <= 8 * M.EPS * M.TF
    # float64: the same formula stays within the derived bound of the fp32 one
    r64 = rays.double()
    c64 = M.unit_positions(u, N, torch.float64)
    ts64, span64, hit64 = M.positions(r64, M.LO, M.HI, M.TN, M.TF, c64)
    assert M.agree_or_grazing(hit, r64, M.LO, M.HI, M.TN, M.TF)
    same = hit == hit64
    err = (ts.double() - ts64).abs()
    assert bool((err[same] <= M.bound(c64, M.TN, M.TF)[same]).all()), float((err[same] / M.bound(c64, M.TN, M.TF)[same]).max())
    # given unit positions carry no rounding of their own
    ts_g = M.positions(rays, M.LO, M.HI, M.TN, M.TF, c)[0].double()
    ts_g64 = M.positions(r64, M.LO, M.HI, M.TN, M.TF, c.double())[0]
    assert bool(((ts_g - ts_g64).abs()[same] <= M.bound(c.double(), M.TN, M.TF, given=True)[same]).all())
    # the unit interval's ends: c = 0 is t0 exactly; c = 1 is t1 to the two roundings in front of the min, never beyond it
    ends = torch.tensor([[0.0, 1.0]]).expand(B, 2)
    te = M.place(span[:, 0], span[:, 1], ends)
    assert torch.equal(te[:, 0], span[:, 0])
    assert bool((te[:, 1] <= span[:, 1]).all()) and float((span[:, 1] - te[:, 1]).max()) <= 2 * M.EPS * M.TF
