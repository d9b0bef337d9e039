"""The per-image colour correction without a GPU: the model (tests/appearance_model.py) and its committed constants, the
exports and prototypes of the five entry points, their argument rules call by call (every call below is refused or is an empty
problem, so nothing is launched; the pointers are fake and 16-byte aligned), the Python surface -- refusals that come before any
launch and any RNG draw -- and the resource usage of csrc/appearance.hip on gfx950."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import appearance_model as AM
import ray_routines_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, ODD, ODD4 = 0x1000, 0x1001, 0x1004          # a 16-byte aligned fake pointer, one aligned to nothing, one to 4 bytes only
EINVAL, EUNSUP = -1, -2
NEW = ("nerf_amd_appearance_gather", "nerf_amd_appearance_apply", "nerf_amd_appearance_apply_backward",
       "nerf_amd_appearance_reduce", "nerf_amd_volume_render_mse_backward_affine")


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_map_and_backward_are_the_autograd_of_the_expression():
    g = torch.Generator().manual_seed(1)
    for dtype in (torch.float32, torch.float64):
        rgb = torch.randn(37, 3, generator=g).to(dtype).requires_grad_(True)
        rows = (0.3 * torch.randn(37, 6, generator=g)).to(dtype).requires_grad_(True)
        up = torch.randn(37, 3, generator=g).to(dtype)
        out = AM.apply(rgb, rows)
        assert torch.equal(out, (1 + rows[:, :3]) * rgb + rows[:, 3:])
        out.backward(up)
        g_rgb, g_rows = AM.apply_backward(up, rgb.detach(), rows.detach())
        assert torch.equal(g_rgb, rgb.grad) and torch.equal(g_rows, rows.grad), dtype
    # theta = 0 is the identity, bit for bit
    c = torch.randn(5, 3, generator=g)
    assert torch.equal(AM.apply(c, torch.zeros(6)), c)


def test_gather_and_reduction_model():
    g = torch.Generator().manual_seed(2)
    theta = torch.randn(4, 6, generator=g)
    ids = torch.tensor([0, 15, 16, 63, 63, -1, 64, 17])
    rows = AM.gather(theta, ids, 16)
    assert torch.equal(rows[:5], theta[[0, 0, 1, 3, 3]]) and torch.equal(rows[7], theta[1])
    assert bool(torch.isnan(rows[5:7]).all()) and not bool(torch.isnan(rows[[0, 1, 2, 3, 4, 7]]).any())
    g_ray = torch.randn(8, 6, generator=g)
    g_ray[5:7] = float("nan")                                 # what a bad ray carries reaches no image
    want, bound = AM.reduce64(g_ray, ids, 16, theta, reg=0.5, frozen=(3,))
    assert np.isfinite(want).all() and not want[3].any() and not bound[3].any()
    assert np.allclose(want[2], 0.5 * theta[2].double().numpy())                          # the absent image: the ridge alone
    assert np.allclose(want[0], (g_ray[0] + g_ray[1]).double().numpy() + 0.5 * theta[0].double().numpy())
    # the bound holds for torch's own fp32 sums in two different orders
    n = 1000
    x = torch.randn(n, 6, generator=g)
    ids = torch.zeros(n, dtype=torch.int64)
    want, bound = AM.reduce64(x, ids, 16, torch.zeros(1, 6))
    fwd = torch.zeros(6)
    for r in x:
        fwd = fwd + r
    for got in (fwd, x.sum(dim=0), x.flip(0).sum(dim=0)):
        assert (np.abs(got.double().numpy() - want[0]) <= bound[0]).all()


def test_reference_fp32_is_inside_the_committed_constants():
    got = AM.measure()
    for g, w in zip(got, (AM.C_REF_APP, AM.C_REF_APP_PLAIN)):
        assert 0.5 * w <= g <= w, (got, AM.C_REF_APP, AM.C_REF_APP_PLAIN)         # recorded, not padded
    assert {N for _, N in AM.head_cases()} == {2, 64, 65, 192} and AM.HEAD_B == 37


def test_cpu_loop_reaches_the_committed_recovery_factors():
    th = AM.recovery_truth()
    assert not th[0].any() and float((1 + th[1:, :3]).min()) >= 0.7 and float((1 + th[1:, :3]).max()) <= 1.3
    assert float(th[:, 3:].abs().max()) <= 0.05 and AM.REC_FROZEN == (0,) and AM.REC_HW == 144
    for fresh, want in ((False, AM.RECOVERY_F_FIXED), (True, AM.RECOVERY_F_FRESH)):
        got = AM.oracle_recovery(fresh)
        assert want <= got <= 1.05 * want, (fresh, got, want)


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_exports_header_and_ctypes_agree(lib):
    from nerf_simple_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    assert lib.nerf_amd_abi_version() == 5 and "#define NERF_AMD_ABI_VERSION 5" in header      # purely additive
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for fn in NEW:
        assert fn in _lib.EXPORTS and hasattr(raw, fn) and getattr(lib, fn).argtypes is not None, fn
        proto = re.search(r"^int " + fn + r"\(([^;]*)\);", header, re.M)
        assert proto, fn
        params = [p.strip() for p in proto.group(1).replace("\n", " ").split(",")]
        res, args = _lib._SIGNATURES[fn]
        assert res is ctypes.c_int and len(params) == len(args), (fn, params)
        for p, a in zip(params, args):      # pointer <-> c_void_p, float <-> c_float, the integer widths
            want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float ") else
                    ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int)
            assert a is want, (fn, p, a)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    # the three-op map lives once, in a header the stages and the head include; no atomics anywhere
    csrc = os.path.join(ROOT, "nerf-simple_amd", "csrc")
    assert "apply_backward" in open(os.path.join(csrc, "appearance_device.h")).read()
    assert '#include "appearance_device.h"' in open(os.path.join(csrc, "composite_backward_device.h")).read()
    for name, uses in (("appearance.hip", '#include "appearance_device.h"'), ("composite_head.hip", "LossHead<BG, DIST, AFFINE>")):
        text = open(os.path.join(csrc, name)).read()
        assert uses in text and "atomicAdd" not in text and "fmaf" not in text, name
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "appearance.hip" in mk and "composite_head.hip" in mk and "appearance_device.h" in mk


# (entry point, arguments, expected code, the rule)
CASES = [
    # gather(theta, ids, ids_copy, HW, theta_ray, B, M)
    ("nerf_amd_appearance_gather", (P, P, None, 16, P, -1, 4), EINVAL, "sizes: B < 0"),
    ("nerf_amd_appearance_gather", (P, P, None, 16, P, 37, 0), EINVAL, "sizes: M <= 0"),
    ("nerf_amd_appearance_gather", (P, P, None, 0, P, 37, 4), EINVAL, "sizes: HW <= 0"),
    ("nerf_amd_appearance_gather", (None, None, None, 16, None, 0, 4), 0, "empty: B == 0 looks at nothing"),
    ("nerf_amd_appearance_gather", (None, None, None, 16, None, 0, 0), EINVAL, "two rules: sizes before the empty problem"),
    ("nerf_amd_appearance_gather", (P, P, None, 16, P, 2 ** 31, 4), EUNSUP, "limits: B"),
    ("nerf_amd_appearance_gather", (P, P, None, 2 ** 31, P, 37, 4), EUNSUP, "limits: HW"),
    ("nerf_amd_appearance_gather", (None, P, None, 16, P, 2 ** 31, 4), EUNSUP, "two rules: limits before pointers"),
    ("nerf_amd_appearance_gather", (None, P, None, 16, P, 37, 4), EINVAL, "pointers: theta"),
    ("nerf_amd_appearance_gather", (P, None, None, 16, P, 37, 4), EINVAL, "pointers: ids"),
    ("nerf_amd_appearance_gather", (P, P, None, 16, None, 37, 4), EINVAL, "pointers: theta_ray"),
    ("nerf_amd_appearance_gather", (ODD4, P, None, 16, P, 37, 4), EINVAL, "alignment: theta"),
    ("nerf_amd_appearance_gather", (P, ODD4, None, 16, P, 37, 4), EINVAL, "alignment: ids"),
    ("nerf_amd_appearance_gather", (P, P, ODD4, 16, P, 37, 4), EINVAL, "alignment: ids_copy"),
    ("nerf_amd_appearance_gather", (P, P, None, 16, ODD4, 37, 4), EINVAL, "alignment: theta_ray"),
    # apply(rgb, theta_ray, theta_stride, out, B)
    ("nerf_amd_appearance_apply", (P, P, 6, P, -1), EINVAL, "sizes: B < 0"),
    ("nerf_amd_appearance_apply", (P, P, 3, P, 37), EINVAL, "sizes: theta_stride"),
    ("nerf_amd_appearance_apply", (P, P, -6, P, 37), EINVAL, "sizes: theta_stride"),
    ("nerf_amd_appearance_apply", (None, None, 0, None, 0), 0, "empty"),
    ("nerf_amd_appearance_apply", (None, None, 5, None, 0), EINVAL, "two rules: sizes before the empty problem"),
    ("nerf_amd_appearance_apply", (P, P, 6, P, 2 ** 31), EUNSUP, "limits: B"),
    ("nerf_amd_appearance_apply", (None, P, 6, P, 37), EINVAL, "pointers: rgb"),
    ("nerf_amd_appearance_apply", (P, None, 0, P, 37), EINVAL, "pointers: theta_ray"),
    ("nerf_amd_appearance_apply", (P, P, 6, None, 37), EINVAL, "pointers: out"),
    ("nerf_amd_appearance_apply", (ODD, P, 6, P, 37), EINVAL, "alignment: rgb"),
    ("nerf_amd_appearance_apply", (P, ODD4, 6, P, 37), EINVAL, "alignment: theta_ray"),
    ("nerf_amd_appearance_apply", (P, P, 6, ODD, 37), EINVAL, "alignment: out"),
    # apply_backward(g_out, rgb, theta_ray, theta_stride, g_rgb, g_theta_ray, B)
    ("nerf_amd_appearance_apply_backward", (P, P, P, 6, P, P, -1), EINVAL, "sizes: B < 0"),
    ("nerf_amd_appearance_apply_backward", (P, P, P, 1, P, P, 37), EINVAL, "sizes: theta_stride"),
    ("nerf_amd_appearance_apply_backward", (None, None, None, 6, None, None, 0), 0, "empty"),
    ("nerf_amd_appearance_apply_backward", (P, P, P, 0, P, P, 2 ** 31), EUNSUP, "limits: B"),
    ("nerf_amd_appearance_apply_backward", (None, P, P, 6, P, P, 37), EINVAL, "pointers: g_out"),
    ("nerf_amd_appearance_apply_backward", (P, None, P, 6, P, P, 37), EINVAL, "pointers: rgb"),
    ("nerf_amd_appearance_apply_backward", (P, P, None, 6, P, P, 37), EINVAL, "pointers: theta_ray"),
    ("nerf_amd_appearance_apply_backward", (P, P, P, 6, None, P, 37), EINVAL, "pointers: g_rgb"),
    ("nerf_amd_appearance_apply_backward", (P, P, P, 6, P, None, 37), EINVAL, "pointers: g_theta_ray"),
    ("nerf_amd_appearance_apply_backward", (ODD, P, P, 6, P, P, 37), EINVAL, "alignment: g_out"),
    ("nerf_amd_appearance_apply_backward", (P, P, ODD4, 6, P, P, 37), EINVAL, "alignment: theta_ray"),
    ("nerf_amd_appearance_apply_backward", (P, P, P, 6, P, ODD4, 37), EINVAL, "alignment: g_theta_ray"),
    # reduce(g_theta_ray, ids, HW, theta, reg, frozen, g_theta, B, M)
    ("nerf_amd_appearance_reduce", (P, P, 16, P, 0.0, None, P, -1, 4), EINVAL, "sizes: B < 0"),
    ("nerf_amd_appearance_reduce", (P, P, 16, P, 0.0, None, P, 37, 0), EINVAL, "sizes: M <= 0"),
    ("nerf_amd_appearance_reduce", (P, P, 16, P, 0.0, None, P, 37, -2), EINVAL, "sizes: M <= 0"),
    ("nerf_amd_appearance_reduce", (P, P, 0, P, 0.0, None, P, 37, 4), EINVAL, "sizes: HW <= 0"),
    ("nerf_amd_appearance_reduce", (P, P, 16, P, -1.0, None, P, 37, 4), EINVAL, "sizes: reg < 0"),
    ("nerf_amd_appearance_reduce", (P, P, 16, P, float("nan"), None, P, 37, 4), EINVAL, "sizes: reg NaN"),
    ("nerf_amd_appearance_reduce", (P, P, 16, P, float("inf"), None, P, 37, 4), EINVAL, "sizes: reg inf"),
    ("nerf_amd_appearance_reduce", (None, None, 16, None, 0.1, None, None, 0, 4), 0, "empty"),
    ("nerf_amd_appearance_reduce", (P, P, 16, P, 0.0, None, P, 37, 2 ** 31), EUNSUP, "limits: M"),
    ("nerf_amd_appearance_reduce", (None, P, 16, P, 0.0, None, P, 37, 4), EINVAL, "pointers: g_theta_ray"),
    ("nerf_amd_appearance_reduce", (P, None, 16, P, 0.0, None, P, 37, 4), EINVAL, "pointers: ids"),
    ("nerf_amd_appearance_reduce", (P, P, 16, None, 0.0, None, P, 37, 4), EINVAL, "pointers: theta"),
    ("nerf_amd_appearance_reduce", (P, P, 16, P, 0.0, None, None, 37, 4), EINVAL, "pointers: g_theta"),
    ("nerf_amd_appearance_reduce", (P, P, 16, P, 0.0, ODD, P, 37, 4), EINVAL, "alignment: frozen"),
    ("nerf_amd_appearance_reduce", (P, P, 16, P, 0.0, None, ODD4, 37, 4), EINVAL, "alignment: g_theta"),
    # head(raw, ts, rays, target, theta_ray, theta_stride, rgb, g_theta_ray, d_raw, B, N)
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, P, P, P, 6, P, P, P, -1, 64), EINVAL, "sizes: B < 0"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, P, P, P, 6, P, P, P, 37, 0), EINVAL, "sizes: N <= 0"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, P, P, P, 12, P, P, P, 37, 64), EINVAL, "sizes: theta_stride"),
    ("nerf_amd_volume_render_mse_backward_affine", (None, None, None, None, None, 6, None, None, None, 0, 64), 0, "empty"),
    ("nerf_amd_volume_render_mse_backward_affine", (None, None, None, None, None, 6, None, None, None, 0, 513), 0,
     "two rules: the empty problem before the limit"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, P, P, P, 6, P, P, P, 37, 513), EUNSUP, "limits: N = 513"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, P, P, P, 7, P, P, P, 37, 513), EINVAL, "two rules: sizes before the limit"),
    ("nerf_amd_volume_render_mse_backward_affine", (None, P, P, P, P, 6, P, P, P, 37, 513), EUNSUP, "two rules: the limit before pointers"),
    # N = 512 is accepted: the call gets past the limit and is refused for its missing pointer
    ("nerf_amd_volume_render_mse_backward_affine", (None, P, P, P, P, 6, P, P, P, 37, 512), EINVAL, "pointers: raw (N = 512 accepted)"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, None, P, P, P, 6, P, P, P, 37, 64), EINVAL, "pointers: ts"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, None, P, P, 6, P, P, P, 37, 64), EINVAL, "pointers: rays"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, P, None, P, 6, P, P, P, 37, 64), EINVAL, "pointers: target"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, P, P, None, 0, P, P, P, 37, 64), EINVAL, "pointers: theta_ray"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, P, P, P, 6, P, None, P, 37, 64), EINVAL, "pointers: g_theta_ray"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, P, P, P, 6, P, P, None, 37, 64), EINVAL, "pointers: d_raw"),
    ("nerf_amd_volume_render_mse_backward_affine", (ODD4, P, P, P, P, 6, P, P, P, 37, 64), EINVAL, "alignment: raw"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, P, P, ODD4, 6, P, P, P, 37, 64), EINVAL, "alignment: theta_ray"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, P, P, P, 6, P, ODD4, P, 37, 64), EINVAL, "alignment: g_theta_ray"),
    ("nerf_amd_volume_render_mse_backward_affine", (P, P, P, P, P, 6, P, P, ODD4, 37, 64), EINVAL, "alignment: d_raw"),
]


def test_cases_cover_every_rule():
    from nerf_simple_amd import _lib
    kinds = {}
    for fn, args, expect, note in CASES:
        assert fn in NEW and len(args) + 1 == len(_lib._SIGNATURES[fn][1]), (fn, note)      # + the stream
        kinds.setdefault(fn, set()).add(note.split(":")[0])
    for fn in NEW:
        assert {"sizes", "empty", "limits", "pointers", "alignment"} <= kinds[fn], (fn, kinds[fn])
        assert {0, EINVAL, EUNSUP} == {c[2] for c in CASES if c[0] == fn}, fn
    head = [c for c in CASES if c[0] == NEW[4]]
    assert {512, 513} <= {a for c in head for a in c[1] if isinstance(a, int)}


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"{CASES[i][0][len('nerf_amd_'):]}-{i}")
def test_abi_refusal(lib, i):
    fn, args, expect, note = CASES[i]
    assert getattr(lib, fn)(*args, None) == expect, (fn, note, args)


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_python_refusals_come_before_any_launch_and_any_draw():
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils.appearance import AppearanceCorrection
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="GPU"):
        AppearanceCorrection(3, 16, device="cpu")
    with pytest.raises(RuntimeError, match="M >= 1"):
        AppearanceCorrection(0, 16)
    with pytest.raises(RuntimeError, match="frozen"):
        AppearanceCorrection(3, 16, frozen=(3,))
    with pytest.raises(RuntimeError, match="frozen"):
        AppearanceCorrection(3, 16, frozen=(-1,))
    with pytest.raises(RuntimeError, match="reg"):
        AppearanceCorrection(3, 16, reg=-0.1)
    app = AppearanceCorrection.__new__(AppearanceCorrection)          # no device here: the argument checks need none
    torch.nn.Module.__init__(app)
    app.M, app.HW, app.theta = 3, 16, torch.nn.Parameter(torch.zeros(3, 6))
    with pytest.raises(RuntimeError, match="GPU"):
        app(torch.zeros(5, 3), torch.zeros(5, dtype=torch.int64))
    rg = object()
    args = (None, None, 64, 8, object())
    for kw, match in ((dict(background=torch.zeros(3)), "background"), (dict(sigma_noise=0.1), "sigma_noise"),
                      (dict(distortion=0.01), "distortion")):
        with pytest.raises(RuntimeError, match=match):
            T.GraphedAppearanceTrainStep(*args, rays_from=rg, **kw)
    with pytest.raises(RuntimeError, match="AppearanceCorrection"):
        T.GraphedAppearanceTrainStep(*args, rays_from=rg)
    with pytest.raises(TypeError, match="rays_from"):
        T.GraphedAppearanceTrainStep(*args)
    assert issubclass(T.GraphedAppearanceTrainStep, T.GraphedTrainStep)
    stepper = T.GraphedAppearanceTrainStep.__new__(T.GraphedAppearanceTrainStep)
    with pytest.raises(RuntimeError, match="takes no rays"):
        stepper.step(torch.zeros(64, 6), torch.zeros(64, 3))
    assert torch.equal(torch.get_rng_state(), state)


def test_a_process_group_is_refused(monkeypatch):
    from nerf_simple_amd import parallel, training as T
    monkeypatch.setattr(parallel, "collectives_active", lambda group=None: True)
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="one replica"):
        T.GraphedAppearanceTrainStep(None, None, 64, 8, object(), rays_from=object())
    assert torch.equal(torch.get_rng_state(), state)


# ---- the compiled kernels --------------------------------------------------------------------------------------------------------
def _scratch_of(source):
    """{demangled kernel name: scratch bytes per lane} of one csrc file compiled for gfx950"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "nerf-simple_amd", "csrc", source)
    out = subprocess.run([hipcc, "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-c", src, "-o", os.devnull,
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert len(names) == len(scratch) == len(set(names)), names
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(plain, scratch))


def test_appearance_kernels_use_no_scratch():
    """For gfx950: csrc/appearance.hip is the four stages, and csrc/composite_head.hip exactly the instantiations
    (NOISE, BG, DIST, AFFINE, E) of the dense head the entry points reach -- the eight without a sampler (E = 0), the affine one
    among them, and the twelve of the pair's coarse head, (NOISE, BG) with a term on at E = 1, 2, 4, 8 --; none with a byte of
    scratch (the head keeps its 8 chunks of per-sample state and the six floats of the ray's row in registers)."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    stages = _scratch_of("appearance.hip")
    assert len(stages) == 4 and all("appearance_" in n for n in stages), stages
    assert set(stages.values()) == {0}, stages
    heads = _scratch_of("composite_head.hip")
    flags = lambda *on: ", ".join("true" if b else "false" for b in on)      # noqa: E731
    want = {flags(0, 1, 0, 0), flags(1, 0, 0, 0), flags(1, 1, 0, 0),         # background and noise
            flags(0, 0, 1, 0), flags(0, 1, 1, 0), flags(1, 0, 1, 0), flags(1, 1, 1, 0),      # with the distortion term
            flags(0, 0, 0, 1)}                                               # the affine head
    got = [re.search(r"dense_head_kernel<([^>]*)>", n).group(1) for n in heads]
    assert {g[:-len(", 0")] for g in got if g.endswith(", 0")} == want, heads
    assert {g for g in got if not g.endswith(", 0")} == \
        {f"{flags(n, b, 0, 0)}, {e}" for n, b in ((0, 1), (1, 0), (1, 1)) for e in (1, 2, 4, 8)}, heads
    assert len(heads) == 20 and len(set(got)) == 20, heads
    assert set(heads.values()) == {0}, heads
    affine = [n for n in heads if f"<{flags(0, 0, 0, 1)}, 0>" in n]
    assert len(affine) == 1 and heads[affine[0]] == 0, heads
