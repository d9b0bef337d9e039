"""The image metrics without a GPU: the float64 definition (tests/ssim_model.py) against an independent restatement, the
committed constant of its fp32 yardstick and the recorded reason for the two-pass kernel, the exports and prototypes of the two
new entry points, their argument rules call by call (tests/golden/abi_refusals_metrics.json, recorded from the library: every
call is refused, is an empty problem or is a size query, so nothing is launched), and the Python surface -- refusals that come
before any launch and any RNG draw."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import ssim_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_refusals_metrics.json")
FAKE = 0x1000
QUERY, METRICS = "nerf_amd_image_metrics_workspace_bytes", "nerf_amd_image_metrics"
NEW = (QUERY, METRICS)

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
    return FAKE if a == "P" else a


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_definition_agrees_with_separable_filtering():
    """Float64 against float64: the windowed definition and scipy's separable correlation with reflect padding, cropped by
    5 -- the uncentred form there, which is harmless in double.  The fp32 window sums to S = 1 - 2.8e-9, not to 1, and the
    definition centres with it: sum G (a - mu_a)(b - mu_b) = sum G a b - (2 - S) mu_a mu_b exactly."""
    ndimage = pytest.importorskip("scipy.ndimage")
    g = SM.window32().astype(np.float64)

    def blur(x):
        return ndimage.correlate1d(ndimage.correlate1d(x, g, axis=0, mode="reflect"), g, axis=1, mode="reflect")[5:-5, 5:-5]

    for kind in SM.CLASSES:
        for H, W in ((11, 11), (16, 19), (33, 47)):
            a, b = (x.astype(np.float64) for x in SM.images(kind, H, W))
            mu_a, mu_b = blur(a), blur(b)
            k = 2.0 - g.sum() ** 2
            s_aa, s_ab, s_bb = blur(a * a) - k * mu_a ** 2, blur(a * b) - k * mu_a * mu_b, blur(b * b) - k * mu_b ** 2
            want = (2 * mu_a * mu_b + SM.C1) * (2 * s_ab + SM.C2) / ((mu_a ** 2 + mu_b ** 2 + SM.C1) * (s_aa + s_bb + SM.C2))
            got = SM.ssim_map64(a, b)
            assert got.shape == (H - 10, W - 10, 3)
            assert float(np.abs(got - want).max()) <= 1e-12, (kind, H, W)


def test_window_is_the_kernels():
    g = SM.window32()
    assert g.dtype == np.float32 and abs(float(g.astype(np.float64).sum()) - 1) < 1e-8 and np.array_equal(g, g[::-1])
    text = open(os.path.join(ROOT, "nerf-simple_amd", "csrc", "image_metrics.hip")).read()
    row = re.search(r"__constant__ float WINDOW\[WIN\] = \{([^}]*)\}", text).group(1)
    assert [float.fromhex(v.strip().rstrip("f")) for v in row.split(",")] == [float(v) for v in g]
    assert re.search(r"constexpr int T = (\d+);", text).group(1) == str(SM.TILE)


def test_yardstick_constant_and_the_reason_for_two_passes():
    got = SM.measure()
    worst = max(c for c, _ in got.values())
    assert 0.5 * SM.C_REF_SSIM <= worst <= SM.C_REF_SSIM, got                 # recorded, not padded
    assert got["identical"] == (0.0, 0.0)
    c, u = got["flat_white"]
    assert u >= 100 * c and u >= 100 * SM.C_REF_SSIM, got                      # E[a^2] - mu^2 cancels on a white background
    assert 0.5 * SM.UNCENTRED_FLAT_WHITE <= u <= 2 * SM.UNCENTRED_FLAT_WHITE
    for kind in SM.CLASSES:                                                    # the classes are what they say
        a, b = SM.images(kind, 16, 19)
        assert a.dtype == b.dtype == np.float32 and a.shape == (16, 19, 3) and 0 <= a.min() and a.max() <= 1
    a, b = SM.images("identical", 16, 19)
    assert a is b
    a, b = SM.images("flat_white", 33, 47)
    assert a.min() >= 0.99 and b.min() >= 0.99


def test_metrics64_restates_the_reference_psnr():
    from nerf_simple_amd import training as T
    a, b = SM.images("noise", 16, 19)
    want = SM.metrics64(a, b)
    got = float(T.img_psnr(torch.from_numpy(b).double(), torch.from_numpy(a).double()))
    # img_psnr divides by log(torch.tensor(10.0)), an fp32 number: half a unit of 2^-23 on either term
    assert abs(got - want["psnr_ref"]) <= 2.0 ** -23 * (abs(20 * np.log10(want["max_gt"])) + abs(want["psnr"])) + 1e-12
    assert abs(float(T.img_mse(torch.from_numpy(b).double(), torch.from_numpy(a).double())) - want["mse"]) <= 1e-15
    same = SM.metrics64(a, a)
    assert same["ssim"] == 1.0 and same["psnr"] == np.inf


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
        for p, a in zip(params, args):      # pointer <-> c_void_p, the integer widths; no scalar double anywhere
            assert "*" in p or not p.startswith("double"), (fn, p)
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int
            assert a is want, (fn, p, a)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    text = open(os.path.join(ROOT, "nerf-simple_amd", "csrc", "image_metrics.hip")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "atomic" not in code and "asm" not in code


def test_size_query(lib):
    q = lib.nerf_amd_image_metrics_workspace_bytes
    for M, H, W in ((1, 1, 1), (1, 11, 11), (3, 70, 45), (8, 800, 800), (1, 1, 2 ** 31 - 1), (2 ** 20, 800, 800)):
        assert q(M, H, W) > 0 and q(M, H, W) % 8 == 0, (M, H, W)
    assert q(2, 70, 45) == 2 * q(1, 70, 45)
    assert q(0, 70, 45) == 0
    assert q(-1, 70, 45) == q(1, 0, 45) == q(1, 70, -3) == -1
    assert q(1, 2, 2 ** 30) == q(1, 65536, 32768) == -2
    assert q(0, 2, 2 ** 30) == 0 and q(-1, 2, 2 ** 30) == -1
    assert q(2 ** 62, 800, 800) == -2                                          # a size that leaves an int64


def test_fixture_covers_every_rule():
    from nerf_simple_amd import _lib
    kinds, two_rules = {}, {}
    for c in CASES:
        assert c["fn"] in NEW and len(c["args"]) == len(_lib._SIGNATURES[c["fn"]][1]), c
        assert c["expect"] in (0, -1, -2) or (c["fn"] == QUERY and c["expect"] > 0), c
        kinds.setdefault(c["fn"], set()).add(c["note"].split(":")[0])
        if c["note"].startswith("two rules:"):
            two_rules[c["fn"]] = two_rules.get(c["fn"], 0) + 1
    assert {"sizes", "empty", "limits", "ssim sizes", "pointers", "alignment", "two rules"} <= kinds[METRICS]
    assert {"sizes", "empty", "limits", "two rules"} <= kinds[QUERY]
    assert two_rules[METRICS] >= 5 and two_rules[QUERY] >= 2
    mine = [c for c in CASES if c["fn"] == METRICS]
    assert {0, -1, -2} == {c["expect"] for c in mine}
    # both sides of every rule: H and W at 10 / 11 with and without SSIM, stride 2 / 3, M -1 / 0 / 1, H W at 2^31 - 1 / 2^31
    seen = {(c["args"][9], c["args"][10], c["args"][5] is not None or c["args"][6] is not None) for c in mine}
    assert {(10, 11, True), (11, 10, True), (11, 11, True), (10, 11, False), (11, 10, False), (10, 10, False)} <= seen
    assert {2, 3} <= {c["args"][1] for c in mine} and {2, 3} <= {c["args"][3] for c in mine}
    assert {-1, 0, 1} <= {c["args"][8] for c in mine}
    assert {(1, 2 ** 31 - 1), (2, 2 ** 30)} <= {(c["args"][9], c["args"][10]) for c in mine}
    for i in (0, 2, 4, 7):                                                     # each required pointer missing
        assert any(c["args"][i] is None and c["note"].startswith("pointers") for c in mine), i
    for i in (0, 2, 4, 5, 6, 7):                                               # each misalignment
        assert any(isinstance(c["args"][i], int) and c["args"][i] % 8 and c["note"].startswith("alignment") for c in mine), i


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"{CASES[i]['fn'][len('nerf_amd_'):]}-{i}")
def test_abi_refusal(lib, i):
    case = CASES[i]
    assert getattr(lib, case["fn"])(*[_arg(a) for a in case["args"]]) == case["expect"], (case["fn"], case["note"], case["args"])


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_python_refusals_come_before_any_launch_and_any_draw():
    from nerf_simple_amd.utils import metrics as MT
    state = torch.get_rng_state()
    img = torch.zeros(16 * 16, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        MT.image_metrics(img, img, 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        MT.ssim(img, img, 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        MT.psnr(img.view(16, 16, 3), img.view(16, 16, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        MT.evaluate_views(lambda pose: img, [np.eye(4)], img, 16, 16)
    # the refusals that depend on the arguments alone come first, the device last: CPU tensors reach every one of them
    f = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype)      # noqa: E731
    for match, pred, gt, H, W, ssim in (
            ("float32", f(256, 3, dtype=torch.float64), f(256, 3), 16, 16, True),
            ("float32", f(256, 3), f(256, 3, dtype=torch.float16), 16, 16, True),
            ("at least 3", f(256, 2), f(256, 3), 16, 16, True),
            ("do not agree", f(2 * 256, 4), f(256, 3), 16, 16, True),
            ("multiple of H W", f(250, 3), f(250, 3), 16, 16, True),
            (r"\[H, W, C\]", f(16, 15, 3), f(16, 15, 3), 16, 16, True),
            ("11 x 11", f(10 * 16, 3), f(10 * 16, 3), 10, 16, True),
            ("11 x 11", f(16 * 10, 3), f(16 * 10, 3), 16, 10, True),
            ("H and W", f(16, 3), f(16, 3), 0, 16, False),
            ("GPU", f(10 * 16, 4), f(10, 16, 3), 10, 16, False),               # all of these are well-formed:
            ("GPU", f(2, 16, 16, 4), f(2 * 256, 3), 16, 16, True),             # only the device is wrong
            ("GPU", f(16, 16, 5), f(16, 16, 3), 16, 16, True)):
        with pytest.raises(RuntimeError, match=match):
            MT.image_metrics(pred, gt, H, W, ssim=ssim)
    with pytest.raises(RuntimeError, match="11 x 11"):
        MT.image_metrics(f(100, 3), f(100, 3), 10, 10, ssim=False, ssim_map=True)
    with pytest.raises(RuntimeError, match=r"gt must be \[len\(poses\) H W, 3\]"):
        MT.evaluate_views(lambda pose: img, [np.eye(4), np.eye(4)], img, 16, 16)
    with pytest.raises(RuntimeError, match="no poses"):
        MT.evaluate_views(lambda pose: img, [], img, 16, 16)

    class Tables:                                           # what RayGenerator.from_tables leaves: no samples, no camera
        samples, cam_params = None, None
    with pytest.raises(RuntimeError, match="evaluate_views"):
        MT.evaluate(None, Tables())

    class Samples:
        samples, cam_params, colours = {"val": [{"transform": np.eye(4)}]}, [16, 16, 20.0], {"val": img}
    with pytest.raises(RuntimeError, match="would go nowhere"):
        MT.evaluate(None, Samples(), render=lambda pose: img, device_rng=True)
    with pytest.raises(RuntimeError, match="im_set"):
        MT.evaluate(None, Samples(), "test")
    with pytest.raises(RuntimeError, match="idxs"):
        MT.evaluate(None, Samples(), idxs=[1])
    with pytest.raises(RuntimeError, match="GPU"):
        MT.evaluate(None, Samples())
    assert torch.equal(torch.get_rng_state(), state)


# ---- recording the fixture ---------------------------------------------------------------------------------------------------
def _build_cases():
    P, A8, A4 = "P", 0x1004, 0x1002            # a fake aligned address; 4 mod 8; 2 mod 4
    out = []

    def m(note, pred=P, ps=4, gt=P, gs=3, sums=P, ssim=P, smap=P, ws=P, M=1, H=16, W=19):
        out.append(dict(fn=METRICS, note=note, args=[pred, ps, gt, gs, sums, ssim, smap, ws, M, H, W, None]))

    def q(note, M, H, W):
        out.append(dict(fn=QUERY, note=note, args=[M, H, W]))

    m("sizes: M < 0", M=-1)
    m("sizes: H <= 0", H=0)
    m("sizes: W <= 0", W=-4)
    m("sizes: pred stride 2", ps=2)
    m("sizes: gt stride 2", gs=2)
    m("sizes: gt stride 0", gs=0)
    m("sizes: strides 3 / 3 pass (then: no workspace)", ps=3, gs=3, ws=None)
    m("empty: M == 0", M=0)
    m("empty: M == 0 with no pointer at all", None, 4, None, 3, None, None, None, None, M=0)
    m("limits: M == 1 passes (then: no sums)", sums=None, M=1)
    m("limits: H W = 2^31 - 1 passes without SSIM (then: no sums)", sums=None, ssim=None, smap=None, H=1, W=2 ** 31 - 1)
    m("limits: H W = 2^31", ssim=None, smap=None, H=2, W=2 ** 30)
    m("limits: H W = 2^31 with SSIM", H=2 ** 16, W=2 ** 15)
    m("limits: the workspace size leaves an int64", M=2 ** 62, H=800, W=800)
    for H, W in ((10, 11), (11, 10), (10, 10)):
        m(f"ssim sizes: {H} x {W} with ssim", smap=None, H=H, W=W)
        m(f"ssim sizes: {H} x {W} with the map alone", ssim=None, H=H, W=W)
        m(f"ssim sizes: {H} x {W} without SSIM passes (then: no gt)", gt=None, ssim=None, smap=None, H=H, W=W)
    m("ssim sizes: 11 x 11 with SSIM passes (then: no pred)", pred=None, H=11, W=11)
    m("ssim sizes: 1 x 1 without SSIM passes (then: no workspace)", ssim=None, smap=None, ws=None, H=1, W=1)
    m("pointers: no pred", pred=None)
    m("pointers: no gt", gt=None)
    m("pointers: no sums", sums=None)
    m("pointers: no workspace", ws=None)
    m("pointers: no workspace, squared error only", ssim=None, smap=None, ws=None)
    m("alignment: pred 2 mod 4", pred=A4)
    m("alignment: gt 2 mod 4", gt=A4)
    m("alignment: sums 4 mod 8", sums=A8)
    m("alignment: ssim 4 mod 8", ssim=A8)
    m("alignment: ssim_map 2 mod 4", smap=A4)
    m("alignment: workspace 4 mod 8", ws=A8)
    m("two rules: sizes before empty (M == 0, stride 2)", ps=2, M=0)
    m("two rules: sizes before limits (W <= 0, H W would be large)", H=2 ** 31 - 1, W=0)
    m("two rules: empty before limits (M == 0, H W = 2^31)", M=0, H=2, W=2 ** 30)
    m("two rules: empty before ssim sizes (M == 0, 10 x 10)", M=0, H=10, W=10)
    m("two rules: limits before ssim sizes (H W = 2^31, W = 2)", H=2 ** 30, W=2)
    m("two rules: ssim sizes before pointers (10 x 11, no pred)", pred=None, H=10, W=11)
    m("two rules: ssim sizes before alignment (11 x 10, sums 4 mod 8)", sums=A8, H=11, W=10)
    m("two rules: pointers before alignment (no gt, pred 2 mod 4)", pred=A4, gt=None)
    m("two rules: sizes before pointers (stride 2, no sums)", gs=2, sums=None)
    q("sizes: M < 0", -1, 16, 19)
    q("sizes: H <= 0", 1, 0, 19)
    q("sizes: W <= 0", 1, 16, 0)
    q("empty: M == 0", 0, 16, 19)
    q("limits: 16 x 19", 1, 16, 19)
    q("limits: 10 x 10 (the query does not know about SSIM)", 1, 10, 10)
    q("limits: H W = 2^31 - 1", 1, 1, 2 ** 31 - 1)
    q("limits: H W = 2^31", 1, 2, 2 ** 30)
    q("limits: the size leaves an int64", 2 ** 62, 800, 800)
    q("two rules: sizes before empty (M == 0, H <= 0)", 0, 0, 19)
    q("two rules: sizes before limits (M < 0, H W = 2^31)", -1, 2, 2 ** 30)
    q("two rules: empty before limits (M == 0, H W = 2^31)", 0, 2, 2 ** 30)
    return out


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    from nerf_simple_amd import _lib
    cases = _build_cases()
    for c in cases:
        c["expect"] = getattr(_lib.lib(), c["fn"])(*[_arg(a) for a in c["args"]])
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]\n")
    print(f"{len(cases)} cases recorded")
