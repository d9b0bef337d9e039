"""The camera optimiser without a GPU: the float64 model (tests/camera_model.py) and the identity the backward kernel
evaluates, the committed constants of its error rules, the exports and prototypes of the new entry points, their argument
rules call by call (tests/golden/abi_refusals_camera.json, recorded from the library: every call is refused, is an empty
problem or is a size query, so nothing is launched), and the Python surface -- refusals that come before any launch and
any RNG draw."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import camera_model as CM
import input_grad_model as IG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_refusals_camera.json")
FAKE = 0x1000
NEW = ("nerf_amd_camera_rays", "nerf_amd_camera_workspace_bytes", "nerf_amd_camera_rays_backward", "nerf_amd_camera_poses")

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


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_batched_table_is_pose_rays_per_image():
    case = next(c for c in CM.cases() if c.M == 3 and c.B == 65 and c.kind == "mixed")
    dirs = CM.camera_dirs(torch.float64)
    for theta in CM.THETAS:
        xi, poses0, _, _ = CM.case_inputs(case, theta)
        pose4 = torch.zeros(case.M, 4, 4, dtype=torch.float64)
        pose4[:, :3] = poses0.double()
        want = torch.cat([IG.pose_rays(xi[m].double(), pose4[m], dirs) for m in range(case.M)])
        got = CM.ray_table(xi.double(), poses0, dirs)
        assert float((got - want).abs().max()) <= 1e-14, theta
    # and the directions are the reference's own table at xi = 0, in fp32 bit for bit
    from nerf_simple_amd.utils.xyz import camera_rays
    pose4 = pose4.float()
    want = camera_rays(pose4, [CM.H, CM.W, CM.F])
    got = CM.ray_table(torch.zeros(case.M, 6), poses0, CM.camera_dirs(torch.float32))
    assert float((got - want).abs().max()) <= 4 * CM.EPS * float(want.abs().max())


def test_left_jacobian_identity_is_the_autograd_of_the_exponential():
    """g_w = J^T sum (y x g_d), g_tau = sum g_o: float64 against float64 autograd through torch.linalg.matrix_exp."""
    for case in (c for c in CM.cases() if c.M == 3 and c.B in (1, 65, 257)):
        for theta in CM.THETAS:
            xi, poses0, ids, g = CM.case_inputs(case, theta)
            _, want, _, unit, _ = CM.model(xi, poses0, ids, g)
            got = CM.identity_grad(xi, poses0, ids, g)
            # float64 against float64: a 2^-20 share of the fp32 unit
            assert CM.ratio(got, want, unit) <= 2.0 ** -20, (case.id, theta)


def test_absent_images_and_bad_ids():
    case = next(c for c in CM.cases() if c.M == 70 and c.B == 65 and c.kind == "ends")
    xi, poses0, ids, g = CM.case_inputs(case, 0.5)
    r, gx, u_r, u_g, _ = CM.model(xi, poses0, ids, g)
    assert not gx[1:-1].any() and not u_g[1:-1].any() and gx[0].any() and gx[-1].any()
    case = next(c for c in CM.cases() if c.M == 3 and c.B == 65 and c.kind == "mixed")
    xi, poses0, ids, g = CM.case_inputs(case, 0.5)
    bad = ~CM.valid_rows(ids, case.M).numpy()
    assert bad.sum() == 2 and {int(i) for i in ids[torch.from_numpy(bad)]} == {-1, case.M * CM.H * CM.W}
    r, gx, _, _, _ = CM.model(xi, poses0, ids, g)
    assert np.isnan(r[bad]).all() and not np.isnan(r[~bad]).any()
    g2 = g.clone()
    g2[torch.from_numpy(bad)] = 1e6                       # what a bad row carries reaches no gradient
    assert np.array_equal(CM.model(xi, poses0, ids, g2)[1], gx)


def test_reference_fp32_is_inside_the_committed_constants():
    got = CM.measure()
    want = (CM.C_REF_CAM_DIR, CM.C_REF_CAM_ORIGIN, CM.C_REF_CAM_GW, CM.C_REF_CAM_GTAU, CM.C_REF_CAM_DIR_COND)
    for g, w in zip(got, want):
        assert 0.5 * w <= g <= w, (got, want)               # recorded, not padded


def test_recovery_constants_are_written_down():
    assert CM.RECOVERY_F_FIXED > 1.8 and CM.RECOVERY_F_FRESH > 2.0 and CM.RECOVERY_N_FRESH == CM.REC_N
    start = CM.recovery_start()
    assert start.shape == (3, 6) and len({tuple(r.tolist()) for r in start}) == 3


# ---- the library -------------------------------------------------------------------------------------------------------------
def test_exports_header_and_ctypes_agree(lib):
    from nerf_simple_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    assert lib.nerf_amd_abi_version() == 5 and "#define NERF_AMD_ABI_VERSION 5" in header      # purely additive
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for fn in NEW:
        assert fn in _lib.EXPORTS and hasattr(raw, fn), fn
        proto = re.search(r"^(int|int64_t) " + fn + r"\(([^;]*)\);", header, re.M)
        assert proto, fn
        params = [p.strip() for p in proto.group(2).replace("\n", " ").split(",")]
        res, args = _lib._SIGNATURES[fn]
        assert res is (ctypes.c_int if proto.group(1) == "int" else ctypes.c_int64) and len(params) == len(args), (fn, params)
        for p, a in zip(params, args):      # pointer <-> c_void_p, float <-> c_float, the integer widths
            want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float ") else
                    ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int)
            assert a is want, (fn, p, a)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    # the per-pose routine lives once, in a header; the kernels call it and state no coefficient of their own
    csrc = os.path.join(ROOT, "nerf-simple_amd", "csrc")
    assert "corrected_pose" in open(os.path.join(csrc, "camera_device.h")).read()
    text = open(os.path.join(csrc, "camera.hip")).read()
    assert text.count("corrected_pose(") == 3 and "sinf" not in text and "atomicAdd" not in text
    assert lib.nerf_amd_camera_workspace_bytes(4096, 100) >= 0


def test_fixture_covers_every_rule():
    from nerf_simple_amd import _lib
    two_rules, kinds = {}, {}
    for c in CASES:
        assert c["fn"] in NEW and len(c["args"]) == len(_lib._SIGNATURES[c["fn"]][1]), c
        assert c["expect"] in (0, -1, -2), c
        kinds.setdefault(c["fn"], set()).add(c["note"].split(":")[0])
        if c["note"].startswith("two rules:"):
            two_rules[c["fn"]] = two_rules.get(c["fn"], 0) + 1
    for fn in NEW[0], NEW[2], NEW[3]:
        # sizes, the empty problem, limits, pointers, alignment -- and every adjacent pair of them in that order
        assert {"sizes", "empty", "limits", "pointers", "alignment", "two rules"} <= kinds[fn], fn
        assert two_rules[fn] >= 4, fn
        mine = [c for c in CASES if c["fn"] == fn]
        assert {0, -1, -2} == {c["expect"] for c in mine}, fn
        assert {2 ** 31 - 1, 2 ** 31} <= {a for c in mine for a in c["args"] if isinstance(a, int)}, fn
    for fn in NEW[0], NEW[2]:
        scalars = {a for c in CASES if c["fn"] == fn for a in c["args"] if isinstance(a, (float, str)) and a != "P"}
        assert {"nan", "inf", 0.0} <= scalars and any(isinstance(a, float) and a < 0 for a in scalars), (fn, scalars)


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"{CASES[i]['fn'][len('nerf_amd_'):]}-{i}")
def test_abi_refusal(lib, i):
    case = CASES[i]
    assert getattr(lib, case["fn"])(*[_arg(a) for a in case["args"]]) == case["expect"], (case["fn"], case["note"], case["args"])


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_python_refusals_come_before_any_launch_and_any_draw():
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils.cameras import CameraRefinement
    state = torch.get_rng_state()
    poses = torch.eye(4).repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        CameraRefinement(poses, [4, 4, 3.0], device="cpu")
    with pytest.raises(RuntimeError, match=r"\[M,4,4\]"):
        CameraRefinement(torch.eye(4), [4, 4, 3.0])
    with pytest.raises(ValueError, match="cam_params"):
        CameraRefinement(poses, [4, 0, 3.0])
    cams, rg = object(), object()
    args = (None, None, 64, 8, cams)
    for kw, match in ((dict(storage="e4m3"), "e4m3"), (dict(buckets=2), "bucket"),
                      (dict(background=torch.zeros(3)), "background"), (dict(sigma_noise=0.1), "sigma_noise"),
                      (dict(distortion=0.01), "distortion")):
        with pytest.raises(RuntimeError, match=match):
            T.GraphedCameraTrainStep(*args, rays_from=rg, **kw)
    with pytest.raises(RuntimeError, match="CameraRefinement"):
        T.GraphedCameraTrainStep(*args, rays_from=rg)
    assert issubclass(T.GraphedCameraTrainStep, T.GraphedTrainStep)
    # step(rays, gt): the rays are the stepper's -- refused before anything else is looked at
    stepper = T.GraphedCameraTrainStep.__new__(T.GraphedCameraTrainStep)
    with pytest.raises(RuntimeError, match="takes no rays"):
        stepper.step(torch.zeros(64, 6), torch.zeros(64, 3))
    assert torch.equal(torch.get_rng_state(), state)


def test_a_process_group_is_refused(monkeypatch):
    from nerf_simple_amd import parallel, training as T
    monkeypatch.setattr(parallel, "collectives_active", lambda group=None: True)
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="one replica"):
        T.GraphedCameraTrainStep(None, None, 64, 8, object(), rays_from=object())
    assert torch.equal(torch.get_rng_state(), state)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    from nerf_simple_amd import _lib
    for c in CASES:
        c["expect"] = getattr(_lib.lib(), c["fn"])(*[_arg(a) for a in c["args"]])
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in CASES) + "\n]\n")
    print(f"{len(CASES)} cases recorded")
