"""Background colour and sigma noise for the dense training path, without a GPU: the exports, the argument rules of the four
new entry points call by call (tests/golden/abi_refusals_background.json, the format of abi_refusals_guided.json: every call
is refused or is an empty problem, so nothing is launched), the Python refusals, which come before any launch and any RNG
draw, the float64 noise model's statistics and the committed constants of the head's error rule (tests/background_model.py)."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import background_model as BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_refusals_background.json")
FAKE = 0x1000
NEW = ("nerf_amd_sigma_noise", "nerf_amd_background_blend", "nerf_amd_background_blend_backward",
       "nerf_amd_volume_render_mse_backward_bg")

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


def test_exports_header_and_ctypes_agree(lib):
    from nerf_simple_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    assert lib.nerf_amd_abi_version() == 5 and "#define NERF_AMD_ABI_VERSION 5" in header      # purely additive
    for fn in NEW:
        assert fn in _lib.EXPORTS and hasattr(lib, fn), fn
        proto = re.search(r"^int " + fn + r"\(([^;]*)\);", header, re.M)
        assert proto, fn
        params = [p.strip() for p in proto.group(1).replace("\n", " ").split(",")]
        res, args = _lib._SIGNATURES[fn]
        assert len(params) == len(args), (fn, params)
        import ctypes
        for p, a in zip(params, args):      # pointer <-> c_void_p, float <-> c_float, the integer widths
            want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float ") else
                    ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_uint64 if p.startswith("uint64_t") else
                    ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
            assert a is want, (fn, p, a)
    assert "rendering.py:63" in header[header.index("nerf_amd_sigma_noise"):]      # the reference's open TODO is cited
    # the key sits beside the sampler's and is distinct from it and from the selection's
    keys = open(os.path.join(ROOT, "nerf-simple_amd", "csrc", "sample_pdf_device.h")).read()
    assert re.search(r"NOISE_KEY = 0x%xull" % BM.NOISE_KEY, keys) and re.search(r"RNG_KEY = 0x%xull" % BM.RNG_KEY, keys)
    assert len({BM.NOISE_KEY, BM.RNG_KEY, BM.SELECT_KEY, 0}) == 4


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
    head = [c for c in CASES if c["fn"] == "nerf_amd_volume_render_mse_backward_bg"]
    assert {512, 513} <= {a for c in head for a in c["args"] if isinstance(a, int)}
    for fn in ("nerf_amd_sigma_noise", "nerf_amd_volume_render_mse_backward_bg"):
        stds = {a for c in CASES if c["fn"] == fn for a in c["args"] if isinstance(a, (float, str)) and a != "P"}
        assert {-1.0, "nan", "inf", 0.0} <= stds, (fn, stds)


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"{CASES[i]['fn'][len('nerf_amd_'):]}-{i}")
def test_abi_refusal(lib, i):
    case = CASES[i]
    assert getattr(lib, case["fn"])(*[_arg(a) for a in case["args"]]) == case["expect"], (case["fn"], case["note"], case["args"])


def test_python_arguments_and_refusals():
    """Keyword-only, off by default, on the dense entry points only; with a grid they are refused before the rays are even
    looked at (CPU tensors here: anything later would raise about the device instead) and before any RNG draw."""
    from nerf_simple_amd import training
    from nerf_simple_amd.utils import rendering
    for fn, names in ((rendering.render_nerf, ("background", "sigma_noise", "noise_seed")),
                      (rendering.volume_render, ("background",)), (rendering.render_view, ("background",)),
                      (training.train_step, ("background", "sigma_noise", "noise_seed")),
                      (training.GraphedTrainStep.__init__, ("background", "sigma_noise", "noise_seed"))):
        sig = inspect.signature(fn).parameters
        for n in names:
            assert sig[n].kind is inspect.Parameter.KEYWORD_ONLY and sig[n].default in (None, 0.0, 0), (fn, n)
    for fn in (training.render_nerf_masked, training.train_step_hierarchical, training.train_step_guided,
               training.GraphedMaskedTrainStep.__init__, training.GraphedHierarchicalTrainStep.__init__,
               training.GraphedMaskedHierarchicalTrainStep.__init__, training.GraphedGuidedTrainStep.__init__,
               rendering.render_view) + tuple(getattr(rendering, n) for n in ("render_hierarchical", "render_hierarchical_view")
                                              if hasattr(rendering, n)):
        sig = inspect.signature(fn).parameters
        assert "sigma_noise" not in sig and (fn is rendering.render_view or "background" not in sig), fn
    assert isinstance(inspect.getattr_static(training.GraphedTrainStep, "sigma_noise"), property)
    assert inspect.getattr_static(training.GraphedTrainStep, "sigma_noise").fset is None          # read-only
    rays, grid = torch.zeros(2, 6), object()
    state = torch.get_rng_state()
    for kw in (dict(background=(1., 1., 1.)), dict(sigma_noise=0.5), dict(background=torch.ones(3), sigma_noise=0.5)):
        for path in (dict(occupancy=grid), dict(terminate=grid), dict(occupancy=grid, terminate=grid)):
            with pytest.raises(RuntimeError, match="dense path only"):
                rendering.render_nerf(rays, None, 8, **kw, **path)
        with pytest.raises(RuntimeError, match="dense path only"):
            training.train_step(None, None, rays, torch.zeros(2, 3), 8, occupancy=grid, **kw)
    for path in (dict(occupancy=grid), dict(terminate=grid)):
        with pytest.raises(RuntimeError, match="dense path only"):
            rendering.render_view(None, None, (4, 4, 1.0), background=(1., 1., 1.), **path)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="standard deviation"):
            rendering.render_nerf(rays, None, 8, sigma_noise=bad)
    with pytest.raises(RuntimeError, match=r"one colour \[3\] or one per ray \[2, 3\]"):
        rendering._background_arg(torch.ones(4, 3), 2, torch.device("cpu"))
    assert rendering._background_arg((1, 0.5, 0), 2, torch.device("cpu"))[1] == 0
    assert rendering._background_arg(torch.ones(2, 3), 2, torch.device("cpu"))[1] == 3
    assert torch.equal(torch.get_rng_state(), state)


def test_noise_model_statistics():
    """The float64 Box-Muller on the oracle's words, 2^16 samples: finite, standard, and uncorrelated with the jitter uniforms
    of the same (seed, ray, i) -- a key shared with the jitter would show there."""
    B, N, seed = 512, 128, 1234
    n = B * N
    z, r = BM.noise_normal(seed, 7, B, N)
    u1, u2 = BM.noise_uniforms(seed, 7, B, N)
    assert n == 2 ** 16 and np.isfinite(z).all() and (u1 > 0).all() and (u1 <= 1).all() and (u2 >= 0).all() and (u2 < 1).all()
    assert abs(z.mean()) <= 5 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / n), z.var()
    u = BM.jitter_uniforms(seed, 7, B, N)
    for name, v in (("z", z), ("u1", u1), ("u2", u2)):
        c = np.corrcoef(v.ravel(), u.ravel())[0, 1]
        assert abs(c) <= 5 / np.sqrt(n), (name, c)
    # the stream moves with the seed and with the step offset, and seed + offset is what keys it
    assert not np.array_equal(z, BM.noise_normal(seed + 1, 7, B, N)[0])
    assert np.array_equal(BM.noise_normal(seed, 7, B, N, offset=3)[0], BM.noise_normal(seed + 3, 7, B, N)[0])
    # batching: rays 7 + 100 .. of this call are rays 107 .. of another
    assert np.array_equal(z[100:], BM.noise_normal(seed, 107, B - 100, N)[0])
    assert BM.K_NOISE == 1.5 * (2 + 3 + 1)


def test_blend_model_edges():
    rgb, acc = torch.tensor([[0.2, float("nan"), 0.9], [0., 0., 0.]]), torch.tensor([1.0 + 2 ** -20, 0.0])
    bg = torch.tensor([1.0, 0.5, 0.25])
    out = BM.blend(rgb, acc, bg)
    assert torch.isnan(out[0, 1]) and float(out[0, 0]) < 0.2 and torch.equal(out[1], bg)      # N == 1: rgb = acc = 0 -> bg
    px = BM.pixels(out, torch.tensor([1.0, float("nan")]))
    assert torch.isnan(px[0, 1]) and torch.isnan(px[1, 3]) and float(px.nan_to_num(0.).max()) <= 1.0


def test_reference_fp32_is_inside_the_committed_constants():
    c_cond, c_plain = BM.measure()
    assert c_cond <= BM.C_REF_BG and c_plain <= BM.C_REF_BG_PLAIN, (c_cond, c_plain)
    assert c_cond >= 0.5 * BM.C_REF_BG and c_plain >= 0.5 * BM.C_REF_BG_PLAIN                 # recorded, not padded
