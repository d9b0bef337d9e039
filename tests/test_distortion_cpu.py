"""The distortion loss without a GPU: the float64 model's algebra and invariances (tests/distortion_model.py), the committed
constants of its error rules, the exports and prototypes of the three entry points, their argument rules call by call
(tests/golden/abi_refusals_distortion.json, recorded from the library: every call is refused or is an empty problem, so nothing
is launched), and the Python surface -- keyword-only arguments that are off by default, and refusals that come before any
launch and any RNG draw."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import distortion_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_refusals_distortion.json")
FAKE = 0x1000
NEW = ("nerf_amd_distortion_loss", "nerf_amd_sum_f32", "nerf_amd_volume_render_mse_backward_dist")

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
    if a == "P":
        return FAKE
    return float(a) if isinstance(a, str) else a


def _some_cases():
    """One case of every (positions, weights) kind at sizes on both sides of a chunk seam."""
    return [c for c in DM.cases() if c.N in (3, 65, 129) and c.B == 5]


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_reference_fp32_is_inside_the_committed_constants():
    c_gw, c_loss = DM.measure()
    assert c_gw <= DM.C_REF_DIST_GW and c_loss <= DM.C_REF_DIST_LOSS, (c_gw, c_loss)
    assert c_gw >= 0.5 * DM.C_REF_DIST_GW and c_loss >= 0.5 * DM.C_REF_DIST_LOSS          # recorded, not padded
    c_cond, c_plain = DM.measure_head()
    assert c_cond <= DM.C_REF_DIST_HEAD and c_plain <= DM.C_REF_DIST_HEAD_PLAIN, (c_cond, c_plain)
    assert c_cond >= 0.5 * DM.C_REF_DIST_HEAD and c_plain >= 0.5 * DM.C_REF_DIST_HEAD_PLAIN


def test_ordered_form_is_the_absolute_form_on_sorted_positions():
    for case in _some_cases():
        ts, w, t_far = DM.inputs(case)
        assert bool((ts[:, 1:] >= ts[:, :-1]).all()), case.id
        D, g, unit_D, unit_g = DM.model(ts, w, t_far)
        wl = w.double().clone().requires_grad_(True)
        Da = DM.direct(ts.double(), wl, t_far)
        Da.sum().backward()
        # float64 against float64: a 2^-29 share of the fp32 unit is rounding noise of either summation order
        assert DM.ratio(Da.detach().numpy(), D, unit_D) <= 2.0 ** -20, case.id
        assert DM.ratio(wl.grad.numpy(), g, unit_g) <= 2.0 ** -20, case.id


def test_prefix_suffix_algebra_is_the_quadratic_sum():
    for case in _some_cases():
        ts, w, t_far = DM.inputs(case)
        D, g, unit_D, unit_g = DM.model(ts, w, t_far)
        Dp, gp = DM.prefix_form(ts, w, t_far)
        assert DM.ratio(Dp.numpy(), D, unit_D) <= 2.0 ** -20 and DM.ratio(gp.numpy(), g, unit_g) <= 2.0 ** -20, case.id


def test_shift_scale_zero_and_single_sample():
    case = next(c for c in DM.cases() if c.N == 65 and c.B == 5 and c.positions == "merged" and c.weights == "rendered")
    ts, w, t_far = DM.inputs(case)
    D, g, unit_D, unit_g = DM.model(ts, w, t_far)
    assert (D > 0).all()
    # exact binary shift and scale of the fp32 positions: D(t + 8) = D(t), D(4 t) = 4 D(t) up to float64 rounding
    Ds, gs, _, _ = DM.model(ts.double() + 8.0, w, t_far + 8.0)
    assert np.allclose(Ds, D, rtol=1e-12, atol=0) and np.allclose(gs, g, rtol=0, atol=1e-12)
    Dk, gk, _, _ = DM.model(ts.double() * 4.0, w, t_far * 4.0)
    assert np.allclose(Dk, 4.0 * D, rtol=1e-13, atol=0) and np.allclose(gk, 4.0 * g, rtol=1e-12, atol=1e-15)
    Dz, gz, uz, _ = DM.model(ts, torch.zeros_like(w), t_far)
    assert not Dz.any() and not gz.any() and not uz.any()
    D1, g1, _, _ = DM.model(ts[:, :1], w[:, :0], t_far)                  # the reference's empty sample axis
    assert D1.shape == (5,) and not D1.any() and g1.shape == (5, 0)


def test_two_clusters_cost_more_than_one():
    ts = torch.linspace(2.0, 6.0, 65)[None, :-1].contiguous()
    one, two = torch.zeros(1, 64), torch.zeros(1, 64)
    one[0, 30:34] = 0.25
    two[0, 10:12] = 0.25
    two[0, 50:52] = 0.25
    assert float(one.sum()) == float(two.sum())
    D_one, D_two = DM.model(ts, one, 6.0)[0][0], DM.model(ts, two, 6.0)[0][0]
    assert D_two > 5 * D_one > 0, (D_one, D_two)


def test_far_plane_clips_the_last_interval():
    ts = torch.tensor([[2.0, 3.0, 7.0]])
    w = torch.tensor([[0.0, 0.0, 1.0]])
    assert DM.model(ts, w, 6.0)[0][0] == 0.0                               # delta = max(6 - 7, 0) = 0: a point mass costs nothing
    assert DM.model(torch.tensor([[2.0, 3.0, 5.0]]), w, 6.0)[0][0] == pytest.approx(1.0 / 3.0)


# ---- the library -------------------------------------------------------------------------------------------------------------
def test_exports_header_and_ctypes_agree(lib):
    from nerf_simple_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    assert lib.nerf_amd_abi_version() == 5 and "#define NERF_AMD_ABI_VERSION 5" in header      # purely additive
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for fn in NEW:
        assert fn in _lib.EXPORTS and hasattr(raw, fn), fn
        proto = re.search(r"^int " + fn + r"\(([^;]*)\);", header, re.M)
        assert proto, fn
        params = [p.strip() for p in proto.group(1).replace("\n", " ").split(",")]
        res, args = _lib._SIGNATURES[fn]
        assert res is ctypes.c_int and len(params) == len(args), (fn, params)
        for p, a in zip(params, args):      # pointer <-> c_void_p, float <-> c_float, the integer widths
            want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float ") else
                    ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_uint64 if p.startswith("uint64_t") else
                    ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
            assert a is want, (fn, p, a)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    # the per-ray routine lives once, in a header both callers include
    csrc = os.path.join(ROOT, "nerf-simple_amd", "csrc")
    assert "distortion_ray" in open(os.path.join(csrc, "composite_dist_device.h")).read()
    for name in ("composite_dist.hip", "composite_backward_device.h"):
        text = open(os.path.join(csrc, name)).read()
        assert "distortion_ray<" in text and "distortion_ray(" not in text, name


def test_fixture_covers_every_rule():
    from nerf_simple_amd import _lib
    two_rules = {}
    for c in CASES:
        assert c["fn"] in NEW and len(c["args"]) == len(_lib._SIGNATURES[c["fn"]][1]), c
        assert c["expect"] in (0, -1, -2), c
        if c["note"].startswith("two rules:"):
            two_rules[c["fn"]] = two_rules.get(c["fn"], 0) + 1
    for fn in NEW:
        assert two_rules.get(fn, 0) >= 2, fn
    for fn in ("nerf_amd_distortion_loss", "nerf_amd_volume_render_mse_backward_dist"):
        mine = [c for c in CASES if c["fn"] == fn]
        assert {512, 513} <= {a for c in mine for a in c["args"] if isinstance(a, int)}
        scalars = {a for c in mine for a in c["args"] if isinstance(a, (float, str)) and a != "P"}
        assert {"nan", "inf", 0.0} <= scalars and any(isinstance(a, float) and a < 0 for a in scalars), (fn, scalars)
        assert {0, -1, -2} == {c["expect"] for c in mine}, fn


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"{CASES[i]['fn'][len('nerf_amd_'):]}-{i}")
def test_abi_refusal(lib, i):
    case = CASES[i]
    assert getattr(lib, case["fn"])(*[_arg(a) for a in case["args"]]) == case["expect"], (case["fn"], case["note"], case["args"])


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_python_arguments_and_refusals():
    from nerf_simple_amd import training
    T = training
    for fn in (T.train_step, T.train_step_guided, T.GraphedTrainStep.__init__, T.GraphedGuidedTrainStep.__init__,
               T.GraphedMaskedTrainStep.__init__, T.GraphedHierarchicalTrainStep.__init__,
               T.GraphedMaskedHierarchicalTrainStep.__init__, T.GraphedMaskedGuidedTrainStep.__init__):
        p = inspect.signature(fn).parameters["distortion"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0.0 and isinstance(p.default, float), fn
    sig = inspect.signature(T.distortion_loss).parameters
    assert list(sig) == ["w", "ts", "tn", "tf"] and sig["tn"].default == 2 and sig["tf"].default == 6
    prop = inspect.getattr_static(T.GraphedTrainStep, "distortion_weight")
    assert isinstance(prop, property) and prop.fset is None                       # read-only

    rays, gt, grid = torch.zeros(2, 6), torch.zeros(2, 3), object()
    state = torch.get_rng_state()
    # with a grid: refused before the rays are even looked at (CPU tensors here: anything later would raise about the device)
    with pytest.raises(RuntimeError, match="dense and guided steps only"):
        T.train_step(None, None, rays, gt, 8, occupancy=grid, distortion=0.01)
    with pytest.raises(RuntimeError, match="dense and guided steps only"):
        T.train_step_guided(None, None, rays, gt, 4, 4, None, occupancy=grid, distortion=0.01)
    # the masked and hierarchical steppers: before their own argument checks, whatever else they are given
    for ctor, args in ((T.GraphedMaskedTrainStep, (None, None, 2, 8, grid, 0.5)),
                       (T.GraphedHierarchicalTrainStep, (None, None, None, 2, 4, 4)),
                       (T.GraphedMaskedHierarchicalTrainStep, (None, None, None, 2, 4, 4, grid, (0.5, 0.5))),
                       (T.GraphedMaskedGuidedTrainStep, (None, None, 2, 4, 4, None, grid, 0.5))):
        with pytest.raises(RuntimeError, match="dense and guided steps only"):
            ctor(*args, distortion=0.01)
        with pytest.raises(ValueError, match="finite and >= 0"):
            ctor(*args, distortion=-0.01)

    # the base constructor, which those classes inherit: the argument cannot slip through a subclass that forwards it
    class Masked(T.GraphedTrainStep):
        _capacities = (1,)

    class Pair(T.GraphedTrainStep):
        _samples = (4, 8)

    class MaskedGuided(T.GraphedGuidedTrainStep):
        _capacities = (1,)

    for cls, args in ((Masked, (None, None, 2, 8)), (Pair, (None, None, 2, 8)), (MaskedGuided, (None, None, 2, 4, 4, None))):
        with pytest.raises(RuntimeError, match="dense and guided steps only"):
            cls(*args, distortion=0.01)
    for bad in (-0.5, float("nan"), float("inf"), float("-inf")):
        for call in (lambda: T.train_step(None, None, rays, gt, 8, distortion=bad),
                     lambda: T.train_step_guided(None, None, rays, gt, 4, 4, None, distortion=bad),
                     lambda: T.GraphedTrainStep(None, None, 2, 8, distortion=bad),
                     lambda: T.GraphedGuidedTrainStep(None, None, 2, 4, 4, None, distortion=bad)):
            with pytest.raises(ValueError, match="finite and >= 0"):
                call()
    assert torch.equal(torch.get_rng_state(), state)
