"""The masked training controls without a GPU (csrc/masked_controls.hip, training.Controls): the exports
and prototypes of the two entry points, their argument rules call by call (tests/golden/abi_refusals_masked_controls.json, written
from the rules in include/nerf_amd.h: every call is refused, is an empty problem or has no live row, so nothing is launched), and
the Python surface -- ``Controls`` as a validated frozen value, ``controls=`` keyword-only and off by default on every entry
point that takes it, and the refusals, which come before any launch and any RNG draw."""
import ctypes
import inspect
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_refusals_masked_controls.json")
FAKE = 0x1000
NEW = ("nerf_amd_sigma_noise_masked", "nerf_amd_volume_render_masked_mse_backward_dist")

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
    """"P": an aligned fake address; "P4" / "P8": the same address off by that many bytes; "nan" / "inf": the float"""
    if isinstance(a, str) and a.startswith("P"):
        return FAKE + int(a[1:] or 0)
    return float(a) if isinstance(a, str) else a


# ---- the library -------------------------------------------------------------------------------------------------------------
def test_exports_header_and_ctypes_agree(lib):
    from nerf_simple_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    assert lib.nerf_amd_abi_version() == 5 and "#define NERF_AMD_ABI_VERSION 5" in header      # purely additive
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for fn in NEW:
        assert fn in _lib.EXPORTS and hasattr(raw, fn), fn
        protos = re.findall(r"^int " + fn + r"\(([^;]*)\);", header, re.M)
        assert len(protos) == 1, fn                                             # declared once
        params = [p.strip() for p in protos[0].replace("\n", " ").split(",")]
        res, args = _lib._SIGNATURES[fn]
        assert res is ctypes.c_int and len(params) == len(args), (fn, params)
        for p, a in zip(params, args):      # pointer <-> c_void_p, float <-> c_float, the integer widths
            want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float ") else
                    ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_uint64 if p.startswith("uint64_t") else
                    ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
            assert a is want, (fn, p, a)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    assert _lib.EXPORTS[-1] == "nerf_amd_volume_render_masked_mse_backward_pdf"      # the new entries sit in front of it
    # the head's arguments: the plain masked head's up to gt, then the terms, then the outputs and sizes
    plain = re.search(r"^int nerf_amd_volume_render_masked_mse_backward\(([^;]*)\);", header, re.M).group(1)
    names = lambda text: [p.strip().split()[-1].lstrip("*") for p in text.replace("\n", " ").split(",")]
    head = names(re.search(r"^int " + NEW[1] + r"\(([^;]*)\);", header, re.M).group(1))
    k = names(plain).index("gt") + 1
    assert head[:k] == names(plain)[:k]
    assert head[k:] == ["bg", "bg_stride", "std", "noise_flags", "noise_seed", "seed_mem", "t_far", "coef", "rgb", "loss_ray",
                        "d_raw_live", "capacity", "B", "N", "stream"]
    # the noise routine lives once, in the header every caller includes
    csrc = os.path.join(ROOT, "nerf-simple_amd", "csrc")
    assert open(os.path.join(csrc, "sigma_noise_device.h")).read().count("float noisy_sigma(") == 1
    text = open(os.path.join(csrc, "masked_controls.hip")).read()
    assert "noisy_sigma(" in text and "float noisy_sigma(" not in text and "philox" not in text
    # the head is the one masked walk (occupancy_train.hip) over the one noise wrapper: no second kernel, struct or launcher
    walk = open(os.path.join(csrc, "occupancy_train.hip")).read()
    assert "__global__" in text and text.count("__global__") == 1 and "nerf_amd_launch_masked_backward(" in text
    assert walk.count("MaskedSamplesBwd{") == 1 and "nerf_noise::Noisy<" in walk and "noisy_sigma(" not in walk
    sources = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")))
    assert "masked_head" not in sources and "MaskedHeadArgs" not in sources and sources.count("struct Noisy") == 1
    assert "masked_controls.hip" in open(os.path.join(csrc, "Makefile")).read()


def test_fixture_covers_every_rule():
    from nerf_simple_amd import _lib
    for fn in NEW:
        mine = [c for c in CASES if c["fn"] == fn]
        assert all(len(c["args"]) == len(_lib._SIGNATURES[fn][1]) and c["expect"] in (0, -1, -2) for c in mine), fn
        assert sum(c["note"].startswith("two rules:") for c in mine) >= 4, fn
        assert {512, 513} <= {a for c in mine for a in c["args"] if isinstance(a, int)}
        scalars = {a for c in mine for a in c["args"] if isinstance(a, (float, str)) and not str(a).startswith("P")}
        assert {"nan", "inf", 0.0} <= scalars and any(isinstance(a, float) and a < 0 for a in scalars), (fn, scalars)
        assert {-1, -2} <= {c["expect"] for c in mine}, fn
        assert any(str(a).startswith("P") and str(a) != "P" for c in mine for a in c["args"]), fn       # a misaligned address
    assert {c["fn"] for c in CASES} == set(NEW)
    assert 0 in {c["expect"] for c in CASES if c["fn"] == NEW[0]}                  # the stage's empty problems launch nothing


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"{CASES[i]['fn'][len('nerf_amd_'):]}-{i}")
def test_abi_refusal(lib, i):
    case = CASES[i]
    assert getattr(lib, case["fn"])(*[_arg(a) for a in case["args"]]) == case["expect"], (case["fn"], case["note"], case["args"])


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_controls_is_a_validated_frozen_value():
    from nerf_simple_amd.training import Controls
    c = Controls()
    assert (c.background, c.sigma_noise, c.noise_seed, c.distortion) == (None, 0.0, 0, 0.0)
    assert list(inspect.signature(Controls).parameters) == ["background", "sigma_noise", "noise_seed", "distortion"]
    c = Controls(background=(1.0, 1.0, 1.0), sigma_noise=0.5, noise_seed=7, distortion=0.01)
    assert (c.sigma_noise, c.noise_seed, c.distortion) == (0.5, 7, 0.01) and isinstance(c.noise_seed, int)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="standard deviation"):          # _check_sigma_noise's own message
            Controls(sigma_noise=bad)
        with pytest.raises(ValueError, match="finite and >= 0"):             # _check_distortion's
            Controls(distortion=bad)
    for name in ("background", "sigma_noise", "noise_seed", "distortion", "anything"):
        with pytest.raises(AttributeError):
            setattr(c, name, 0)
    with pytest.raises(AttributeError):
        del c.sigma_noise
    d = c.replace(noise_seed=8)
    assert d is not c and d.noise_seed == 8 and d.sigma_noise == 0.5 and c.noise_seed == 7
    with pytest.raises(ValueError):
        c.replace(sigma_noise=-1.0)


def _entry_points():
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils import rendering as R
    return (T.render_nerf_masked, T.train_step, T.train_step_guided, T.GraphedTrainStep.__init__,
            T.GraphedMaskedTrainStep.__init__, T.GraphedMaskedGuidedTrainStep.__init__, R.render_nerf, R.render_view)


def test_controls_is_keyword_only_and_off_by_default():
    for fn in _entry_points():
        p = inspect.signature(fn).parameters["controls"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn
    from nerf_simple_amd.utils import metrics
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(metrics.evaluate).parameters.values())


def test_flat_keywords_and_controls_together_are_refused():
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils import rendering as R
    rays, gt, c = torch.zeros(2, 6), torch.zeros(2, 3), T.Controls(sigma_noise=0.5)
    state = torch.get_rng_state()
    flats = (dict(background=(1., 1., 1.)), dict(sigma_noise=0.5), dict(noise_seed=3), dict(distortion=0.01))
    for kw in flats:
        with pytest.raises(ValueError, match="one of the two"):
            T.train_step(None, None, rays, gt, 8, controls=c, **kw)
        with pytest.raises(ValueError, match="one of the two"):
            T.GraphedTrainStep(None, None, 2, 8, controls=c, **kw)
    for kw in flats[:3]:
        with pytest.raises(ValueError, match="one of the two"):
            R.render_nerf(rays, None, 8, controls=c, **kw)
    with pytest.raises(ValueError, match="one of the two"):
        R.render_view(None, None, (4, 4, 1.0), controls=c, background=(1., 1., 1.))
    with pytest.raises(ValueError, match="one of the two"):
        T.train_step_guided(None, None, rays, gt, 4, 4, None, controls=c, distortion=0.01)
    # not a Controls
    for call in (lambda: T.train_step(None, None, rays, gt, 8, controls=(None, 0.5)),
                 lambda: T.render_nerf_masked(rays, None, 8, object(), controls={"sigma_noise": 0.5}),
                 lambda: T.GraphedMaskedTrainStep(None, None, 2, 8, object(), 0.5, controls=0.5),
                 lambda: R.render_nerf(rays, None, 8, controls="white")):
        with pytest.raises(TypeError, match="training.Controls"):
            call()
    assert torch.equal(torch.get_rng_state(), state)


def test_out_of_scope_paths_refuse_before_any_draw():
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils import rendering as R
    rays, gt, grid = torch.zeros(2, 6), torch.zeros(2, 3), object()
    c = T.Controls(background=(1., 1., 1.), sigma_noise=0.5, distortion=0.01)
    bg = T.Controls(background=(1., 1., 1.))
    cases = [
        ("render_nerf with terminate", RuntimeError, lambda: R.render_nerf(rays, None, 8, terminate=grid, controls=bg)),
        ("render_nerf with a grid and terminate", RuntimeError,
         lambda: R.render_nerf(rays, None, 8, occupancy=grid, terminate=grid, controls=bg)),
        ("render_view with terminate", RuntimeError,
         lambda: R.render_view(None, None, (4, 4, 1.0), occupancy=grid, terminate=grid, controls=bg)),
        ("the eager pair", RuntimeError, lambda: T.train_step_hierarchical(None, None, None, rays, gt, 4, 4, controls=c)),
        ("the eager masked pair", RuntimeError,
         lambda: T.train_step_hierarchical(None, None, None, rays, gt, 4, 4, occupancy=grid, controls=c)),
        ("the graphed pair", RuntimeError, lambda: T.GraphedHierarchicalTrainStep(None, None, None, 2, 4, 4, controls=c)),
        ("the graphed masked pair", RuntimeError,
         lambda: T.GraphedMaskedHierarchicalTrainStep(None, None, None, 2, 4, 4, grid, (0.5, 0.5), controls=c)),
        ("the camera stepper", RuntimeError, lambda: T.GraphedCameraTrainStep(None, None, 2, 8, None, controls=c)),
        ("the appearance stepper", RuntimeError,
         lambda: T.GraphedAppearanceTrainStep(None, None, 2, 8, None, rays_from=None, controls=c)),
        ("a masked stepper in 8-bit storage", ValueError,
         lambda: T.GraphedMaskedTrainStep(None, None, 2, 8, grid, 0.5, storage="e4m3", controls=c)),
        ("a masked guided stepper in 8-bit storage", ValueError,
         lambda: T.GraphedMaskedGuidedTrainStep(None, None, 2, 4, 4, None, grid, 0.5, storage="e4m3", controls=c)),
        # a render is no step: the distortion term is refused; noise behind a grid is the regulariser's refusal
        ("render_nerf_masked with the term", ValueError, lambda: T.render_nerf_masked(rays, None, 8, grid, controls=c)),
        ("render_nerf with the term", ValueError, lambda: R.render_nerf(rays, None, 8, occupancy=grid, controls=c)),
        ("render_view with the term", ValueError, lambda: R.render_view(None, None, (4, 4, 1.0), occupancy=grid, controls=c)),
        ("render_nerf with noise behind a grid", RuntimeError,
         lambda: R.render_nerf(rays, None, 8, occupancy=grid, controls=T.Controls(sigma_noise=0.5))),
        ("render_view with noise behind a grid", RuntimeError,
         lambda: R.render_view(None, None, (4, 4, 1.0), occupancy=grid, controls=T.Controls(sigma_noise=0.5))),
        # the dense guided step knows the distortion term only
        ("the dense guided step with a background", RuntimeError,
         lambda: T.train_step_guided(None, None, rays, gt, 4, 4, None, controls=bg)),
        ("the dense guided stepper with noise", RuntimeError,
         lambda: T.GraphedGuidedTrainStep(None, None, 2, 4, 4, None, controls=T.Controls(sigma_noise=0.5))),
    ]
    for what, exc, call in cases:
        state = torch.get_rng_state()
        with pytest.raises(exc, match="controls|regulariser|storage|distortion"):
            call()
        assert torch.equal(torch.get_rng_state(), state), what
    # the flat keywords keep refusing next to a grid, whatever the bundle can do
    with pytest.raises(RuntimeError, match="dense and guided steps only"):
        T.GraphedMaskedTrainStep(None, None, 2, 8, grid, 0.5, distortion=0.01)
    with pytest.raises(RuntimeError, match="dense path only"):
        T.train_step(None, None, rays, gt, 8, occupancy=grid, background=(1., 1., 1.))
    for fn in (T.render_nerf_masked, T.train_step_guided, T.train_step_hierarchical, T.GraphedMaskedTrainStep.__init__,
               T.GraphedMaskedGuidedTrainStep.__init__):
        sig = inspect.signature(fn).parameters
        assert "background" not in sig and "sigma_noise" not in sig, fn
