"""The training controls of the coarse + fine pair without a GPU (csrc/composite_head.hip, csrc/masked_controls.hip,
training.train_step_hierarchical / the two graphed pair steppers / rendering.render_hierarchical[_view] with ``controls=``;
DESIGN.md section 35): the exports and prototypes of the two coarse heads, their argument rules call by call
(tests/golden/abi_refusals_pair_controls.json, written from the rules in include/nerf_amd.h: every call is refused or is an empty
problem, so nothing is launched), and the Python surface -- ``controls=`` keyword-only and off by default on the six pair entry
points, the order of the refusals (all before any look at the networks and any RNG draw), and the seed rule's constant."""
import ctypes
import inspect
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_refusals_pair_controls.json")
FAKE = 0x1000
DENSE, MASKED = "nerf_amd_volume_render_mse_backward_pdf_bg", "nerf_amd_volume_render_masked_mse_backward_pdf_bg"
NEW = (DENSE, MASKED)
TERMS = ["bg", "bg_stride", "std", "noise_flags", "noise_seed", "seed_mem"]

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


def _names(header, fn):
    protos = re.findall(r"^int " + fn + r"\(([^;]*)\);", header, re.M)
    assert len(protos) == 1, fn                                                 # declared once
    return [p.strip() for p in protos[0].replace("\n", " ").split(",")]


# ---- the library -------------------------------------------------------------------------------------------------------------
def test_exports_header_and_ctypes_agree(lib):
    from nerf_simple_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    assert lib.nerf_amd_abi_version() == 5 and "#define NERF_AMD_ABI_VERSION 5" in header      # purely additive
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for fn in NEW:
        assert fn in _lib.EXPORTS and hasattr(raw, fn), fn
        params = _names(header, fn)
        res, args = _lib._SIGNATURES[fn]
        assert res is ctypes.c_int and len(params) == len(args), (fn, params)
        for p, a in zip(params, args):      # pointer <-> c_void_p, float <-> c_float, the integer widths
            want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float ") else
                    ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_uint64 if p.startswith("uint64_t") else
                    ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
            assert a is want, (fn, p, a)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    assert _lib.EXPORTS[-1] == "nerf_amd_volume_render_masked_mse_backward_pdf"      # the new entries sit in front of it
    # each head's arguments: the plain coarse head's, with the term block where the _bg / _dist heads put theirs
    last = lambda params: [p.split()[-1].lstrip("*") for p in params]      # noqa: E731
    for fn, plain, after in ((DENSE, "nerf_amd_volume_render_mse_backward_pdf", "target"),
                             (MASKED, "nerf_amd_volume_render_masked_mse_backward_pdf", "gt")):
        want = last(_names(header, plain))
        k = want.index(after) + 1
        assert last(_names(header, fn)) == want[:k] + TERMS + want[k:], fn
    for fn, after in (("nerf_amd_volume_render_mse_backward_bg", "target"), ("nerf_amd_volume_render_masked_mse_backward_dist", "gt")):
        names = last(_names(header, fn))
        k = names.index(after) + 1
        assert names[k:k + 3] == TERMS[:3] and names[k + 5] == "seed_mem", fn
    # the launchers are declared once, in the header every caller includes; the noise and the walk are not restated
    csrc = os.path.join(ROOT, "nerf-simple_amd", "csrc")
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    assert sum(t.count("int nerf_amd_launch_dense_head_pdf(") for t in sources.values()) == 2          # declaration + definition
    assert "int nerf_amd_launch_dense_head_pdf(" in sources["launchers.h"]
    pair = sources["composite_head.hip"]
    assert pair.count("__global__") == 1 and "composite_backward_ray<" in pair and "nerf_noise::Noisy<" in pair
    assert "PdfSink" in pair and "philox" not in pair and "atomicAdd" not in pair
    # the sampler is reached through the routine the plain coarse head shares, and only there
    assert "sample_behind_walk<E>" in pair and "sample_behind_walk<E>" in sources["composite.hip"]
    assert "sample_ray<E>" in sources["sample_pdf_device.h"] and "void sample_behind_walk(" in sources["sample_pdf_device.h"]
    assert "sample_ray<" not in pair and "sample_ray<" not in sources["composite.hip"]
    # the old layout is gone: no source, Makefile rule or comment under csrc/ names it
    everything = dict(sources, Makefile=open(os.path.join(csrc, "Makefile")).read())
    assert "composite_head.hip" in everything["Makefile"] and not os.path.exists(os.path.join(csrc, "composite_pair.hip"))
    for f, text in everything.items():
        assert "composite_pair.hip" not in text and "NERF_MASKED_PAIR" not in text, f
    walk = sources["occupancy_train.hip"]
    assert "E == 0 || (Up::MSE && !Up::DIST && !Up::AFFINE)" in walk


def test_keys_per_lane_is_switched_over_once():
    """Nf -> the compile-time E of a launch is one host helper (sample_pdf_device.h with_keys_per_lane): under csrc/ a
    `switch` over keys_per_lane( occurs exactly once, there, and every launcher with a sampler goes through the helper (the
    masked walk's once for its plain and its term heads)."""
    csrc = os.path.join(ROOT, "nerf-simple_amd", "csrc")
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    switches = {f: len(re.findall(r"\bswitch\s*\([^)]*keys_per_lane\(", t)) for f, t in sources.items()}
    assert {f: n for f, n in switches.items() if n} == {"sample_pdf_device.h": 1}, switches
    helper = sources["sample_pdf_device.h"]
    assert helper.index("void with_keys_per_lane(") < helper.index("switch (keys_per_lane(")
    calls = {f: t.count("with_keys_per_lane(") for f, t in sources.items() if f.endswith(".hip")}
    assert {f: n for f, n in calls.items() if n} == {"composite.hip": 1, "composite_head.hip": 1, "occupancy_train.hip": 1,
                                                     "sample_pdf.hip": 1, "guided_sample.hip": 1, "guided_masked.hip": 1}, calls
    # no other ladder over the four buckets: a kernel's E is never spelled as a literal 1, 2, 4 or 8 at a launch
    assert not [f for f, t in sources.items() if re.search(r"_kernel<[^>;]*\b[1248]>\)?, grid", t)], sources.keys()


def test_fixture_covers_every_rule():
    from nerf_simple_amd import _lib
    for fn in NEW:
        mine = [c for c in CASES if c["fn"] == fn]
        assert all(len(c["args"]) == len(_lib._SIGNATURES[fn][1]) and c["expect"] in (0, -1, -2) for c in mine), fn
        assert sum(c["note"].startswith("two rules:") for c in mine) >= 6, fn
        ints = {a for c in mine for a in c["args"] if isinstance(a, int)}
        assert {2, 256, 257} <= ints, (fn, ints)                                 # the sampler's limits from both sides
        scalars = {a for c in mine for a in c["args"] if isinstance(a, (float, str)) and not str(a).startswith("P")}
        assert {"nan", "inf", 0.0} <= scalars and any(isinstance(a, float) and a < 0 for a in scalars), (fn, scalars)
        assert {-1, -2} <= {c["expect"] for c in mine}, fn
        assert any(str(a).startswith("P") and str(a) != "P" for c in mine for a in c["args"]), fn       # a misaligned address
    assert {c["fn"] for c in CASES} == set(NEW)
    assert 0 in {c["expect"] for c in CASES if c["fn"] == DENSE}                 # the dense head's empty problem launches nothing
    assert 0 not in {c["expect"] for c in CASES if c["fn"] == MASKED}            # no capacity fits an empty batch


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"{CASES[i]['fn'][len('nerf_amd_'):]}-{i}")
def test_abi_refusal(lib, i):
    case = CASES[i]
    assert getattr(lib, case["fn"])(*[_arg(a) for a in case["args"]]) == case["expect"], (case["fn"], case["note"], case["args"])


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def _pair_entry_points():
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils import rendering as R
    return (T.train_step_hierarchical, T.GraphedHierarchicalTrainStep.__init__, T.GraphedMaskedHierarchicalTrainStep.__init__,
            R.render_hierarchical, R.render_hierarchical_view)


def test_controls_is_keyword_only_and_off_by_default():
    for fn in _pair_entry_points():
        params = inspect.signature(fn).parameters
        p = params["controls"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn
        assert not {"background", "sigma_noise", "noise_seed"} & set(params), fn       # everything enters through controls=


def test_the_fine_noise_offset():
    from nerf_simple_amd import training as T
    assert T.FINE_NOISE_OFFSET == 1 << 63
    c = T.Controls(sigma_noise=0.5, noise_seed=(1 << 63) + 5)
    from nerf_simple_amd.utils.controls import pair, resolve
    assert pair(c, "a test") is c                 # the coarse pass takes the bundle as it is ...
    coarse = resolve(c, 2, torch.device("cpu"), 9)
    fine = coarse.fine()                                      # ... the fine pass its record under the offset key
    assert coarse.noise_seed == (1 << 63) + 5 and fine.noise_seed == 5 and fine.std == 0.5            # mod 2^64
    assert fine._replace(noise_seed=coarse.noise_seed) == coarse and fine.noise_ray_id0 == 9
    assert pair(None, "a test") is None and pair(T.Controls(), "a test") is None


def _calls(c):
    """the four pair training entry points (eager dense / masked, graphed dense / masked) with ``controls=c`` and None networks"""
    from nerf_simple_amd import training as T
    rays, gt, grid = torch.zeros(2, 6), torch.zeros(2, 3), object()
    return [
        ("the eager pair", lambda: T.train_step_hierarchical(None, None, None, rays, gt, 4, 4, controls=c)),
        ("the eager masked pair", lambda: T.train_step_hierarchical(None, None, None, rays, gt, 4, 4, occupancy=grid, controls=c)),
        ("the graphed pair", lambda: T.GraphedHierarchicalTrainStep(None, None, None, 2, 4, 4, controls=c)),
        ("the graphed masked pair", lambda: T.GraphedMaskedHierarchicalTrainStep(None, None, None, 2, 4, 4, grid, (0.5, 0.5), controls=c)),
    ]


def test_refusal_order_before_the_networks_and_any_draw():
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils import rendering as R
    rays, grid = torch.zeros(2, 6), object()
    state = torch.get_rng_state()
    # 1. not a Controls: TypeError, on all six
    for bad in ((None, 0.5), {"sigma_noise": 0.5}, "white", 0.5):
        for what, call in _calls(bad):
            with pytest.raises(TypeError, match="training.Controls"):
                call()
        for kw in ({}, {"occupancy": grid}):
            with pytest.raises(TypeError, match="training.Controls"):
                R.render_hierarchical(rays, None, None, 4, 4, controls=bad, **kw)
            with pytest.raises(TypeError, match="training.Controls"):
                R.render_hierarchical_view(None, None, None, (4, 4, 1.0), 4, 4, controls=bad, **kw)
    # 2. the distortion term: RuntimeError naming controls= and the term, whatever else the bundle holds
    for c in (T.Controls(distortion=0.01), T.Controls(background=(1., 1., 1.), sigma_noise=0.5, distortion=0.01)):
        for what, call in _calls(c):
            with pytest.raises(RuntimeError, match=r"controls=.*distortion"):
                call()
    # ... and the flat keyword of the two steppers keeps its own refusal
    with pytest.raises(RuntimeError, match="dense and guided steps only"):
        T.GraphedHierarchicalTrainStep(None, None, None, 2, 4, 4, distortion=0.01)
    with pytest.raises(RuntimeError, match="dense and guided steps only"):
        T.GraphedMaskedHierarchicalTrainStep(None, None, None, 2, 4, 4, grid, (0.5, 0.5), distortion=0.01)
    # 3. the renders: a render is no step (ValueError); noise is a regulariser (RuntimeError)
    for kw in ({}, {"occupancy": grid}):
        for c, exc in ((T.Controls(distortion=0.01), ValueError), (T.Controls(sigma_noise=0.5, distortion=0.01), ValueError),
                       (T.Controls(sigma_noise=0.5), RuntimeError), (T.Controls(background=(1., 1., 1.), sigma_noise=0.5), RuntimeError)):
            with pytest.raises(exc, match="distortion|regulariser"):
                R.render_hierarchical(rays, None, None, 4, 4, controls=c, **kw)
            with pytest.raises(exc, match="distortion|regulariser"):
                R.render_hierarchical_view(None, None, None, (4, 4, 1.0), 4, 4, controls=c, **kw)
    assert torch.equal(torch.get_rng_state(), state)


def test_a_bundle_that_is_in_scope_goes_on_to_the_usual_checks():
    """background / sigma noise pass the controls rules: what raises next is the entry point's own first check (None networks),
    not a refusal of the bundle -- and still nothing was drawn."""
    from nerf_simple_amd import training as T
    state = torch.get_rng_state()
    for c in (T.Controls(background=(1., 1., 1.)), T.Controls(sigma_noise=0.5, noise_seed=3)):
        for what, call in _calls(c):
            with pytest.raises(Exception) as e:
                call()
            assert "controls" not in str(e.value), (what, str(e.value))
    assert torch.equal(torch.get_rng_state(), state)
