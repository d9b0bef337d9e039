"""The per-element models of tests/ray_routines_model.py against the oracle, on the CPU: the float64 closed forms equal
the float64 oracle (autograd through oracle.volume_render, oracle.sample_pdf), and the float32 oracle stays inside the
recorded c_ref constants, the judged-row condition and the kink caps on every committed case.  The GPU tests of
tests/test_gpu_ray_routines.py hold the kernels to  2 c_ref + 4  of the same units."""
import numpy as np
import pytest
import torch

import ray_routines_model as M


@pytest.fixture(scope="module")
def measured():
    return M.measure()


def test_closed_forms_equal_the_float64_oracle(oracle):
    """Every kind of upstream gradient on every case: the closed-form backward is the float64 autograd of
    oracle.volume_render to float64 round-off (8 units of 2^-53 A: the first-order bound, in float64's epsilon), and the
    two single-term forms are that same closed form.  Where autograd is not finite the ray is empty (acc == 0)."""
    for case in M.comp_cases():
        raw, ts, d = M.comp_inputs(case)
        fw = M.forward64(raw, ts, d)
        for kind in ("alpha", "w", "rgb", "disp", "acc", "all"):
            g = M.coefs(case, kind, fw)
            want, A = M.model_backward(fw, raw, ts, g)
            assert np.isfinite(want).all() and np.isfinite(A).all() and (A >= 0).all(), (case.id, kind)
            ref = M.oracle_grad(raw, ts, d, g, torch.float64)
            bad = ~np.isfinite(ref).all(axis=(1, 2))
            assert (fw["w"].sum(dim=1).numpy()[bad] == 0).all(), (case.id, kind)
            err = np.abs(want - np.where(np.isfinite(ref), ref, want))
            assert (err <= 8 * 2.0 ** -53 * A).all(), (case.id, kind, float((err / (2.0 ** -53 * A + 1e-300)).max()))
            if kind == "alpha":
                single, unit = M.model_alpha(fw, g[2])
            elif kind == "w":
                single, unit = M.model_w(fw, M.pick_w_samples(fw)[0])
            else:
                continue
            assert (np.abs(single - want) <= 8 * 2.0 ** -53 * A).all(), (case.id, kind)
            assert (single[..., :3] == 0).all() and (ref[..., :3] == 0).all(), (case.id, kind)
            if kind == "w":                      # behind the one-hot sample the reference is exactly zero
                assert (ref[..., 3][unit == 0] == 0).all(), case.id


def test_sampler_model_is_the_float64_oracle(oracle):
    for case in M.pdf_cases():
        ts, w, u = M.pdf_inputs(case)
        want, unit, kink = M.model_pdf(ts, w, u)
        assert np.array_equal(want, oracle.sample_pdf(ts.double(), w.double(), u.double()).numpy()), case.id
        assert (unit > 0).all() and want.shape == (M.PDF_B, case.Nc + case.Nf)


def test_reference_stays_inside_its_c_ref(measured):
    """The constants of the model module are what `python tests/ray_routines_model.py` measures, rounded up."""
    m = measured
    print({k: v for k, v in m.items() if k.startswith("C_REF")})
    for k in ("benign", "dense", "threshold"):
        assert m["C_REF_ALPHA"][k] <= M.C_REF_ALPHA[k] and m["C_REF_W"][k] <= M.C_REF_W[k], k
    assert m["C_REF_ALPHA_COND"] <= M.C_REF_ALPHA_COND and m["C_REF_W_COND"] <= M.C_REF_W_COND
    for k in ("rgb", "disp", "acc", "all"):
        assert m["C_REF_RAY"][k] <= M.C_REF_RAY[k] and m["C_REF_RAY_PLAIN"][k] <= M.C_REF_RAY_PLAIN[k], k
    assert m["C_REF_NONFINITE"] <= M.C_REF_NONFINITE
    assert m["C_REF_PDF"] <= M.C_REF_PDF
    # a constant that the reference does not come near would hand the kernel room nobody measured
    assert m["C_REF_PDF"] >= 0.9 * M.C_REF_PDF and m["C_REF_ALPHA_COND"] >= 0.9 * M.C_REF_ALPHA_COND


def test_judged_rows_and_kink_caps(measured):
    for cid, share in measured["judged_share"].items():
        assert share >= 0.5 or cid in M.W_UNDERJUDGED, (cid, share)
    assert set(M.W_UNDERJUDGED) <= set(measured["judged_share"])
    # the plain per-ray scale judges a fair share of the ray blocks of every kind
    for kind, (judged, total) in measured["plain_judged"].items():
        assert judged >= 0.5 * total, (kind, judged, total)
    for case in M.pdf_cases():
        assert measured["kinks"][case.id] <= M.kink_cap(case) * M.PDF_B, (case.id, measured["kinks"][case.id])


def test_seams_are_covered():
    """The shapes the kernels branch on: the compositor's 64-sample chunks and its N <= 512 limit, ragged last
    workgroups (4 rays each), the sampler's keys-per-lane buckets (Nf = 64 | 65, 128 | 129, 256 | 257) and the cdf scan's
    chunk carry (Nc - 2 bins: 64 | 65 | 128 | 192 at Nc = 66, 67, 130, 194)."""
    cases = M.comp_cases()
    assert {c.N for c in cases} == {2, 3, 63, 64, 65, 128, 129, 300, 512}
    for N in M.COMP_N:
        assert {c.B for c in cases if c.N == N} == {1, 5, 37}
        assert {c.coincident for c in cases if c.N == N} == {False, True}
    assert {(c.Nc, c.Nf) for c in M.pdf_cases()} == {(3, 1), (64, 128), (66, 65), (67, 64), (130, 129), (194, 257), (256, 256)}
    ts, w, u = M.pdf_inputs(M.pdf_cases()[-1])
    assert (u == 0).any() and (u == 1 - M.EPS).any() and (u[:, 17] == u[:, 90]).all()


def test_disparity_edges_in_the_reference(oracle):
    """g_disp alone on the clamp branch and on empty rays, as autograd sees them: zero slope on the clamp branch (the
    constant wins torch.max), NaN on an empty ray (0/0).  The model, like the kernel, gives zero on both."""
    raw, ts, d, g_disp, kinds = M.disp_edge_inputs()
    g = [None, g_disp, None, None, None]
    for dtype in (torch.float32, torch.float64):
        out = oracle.volume_render(raw.to(dtype), ts.to(dtype), d.to(dtype))
        ref = M.oracle_grad(raw, ts, d, g, dtype)
        q = (out[4] * ts.to(dtype)).sum(dim=1) / out[3]
        for r, k in enumerate(kinds):
            if k.startswith("clamp"):
                assert float(q[r]) <= 1e-10 and (ref[r] == 0).all(), (r, k)
            elif k == "empty":
                assert float(out[3][r]) == 0 and np.isnan(ref[r, :, 3]).all() and (ref[r, :, :3] == 0).all(), (r, k)
            else:
                assert float(q[r]) > 1 and np.isfinite(ref[r]).all() and np.abs(ref[r, :, 3]).max() > 0, (r, k)
    want, _ = M.model_backward(M.forward64(raw, ts, d), raw, ts, g)
    plain = np.array([k == "plain" for k in kinds])
    assert (want[~plain] == 0).all() and np.allclose(want[plain], ref[plain], rtol=1e-9, atol=1e-300)


def test_non_finite_inputs_have_clean_rays():
    for k in range(len(M.NONFINITE_SHAPES)):
        raw, ts, d, g_rgb, clean = M.nonfinite_inputs(k)
        assert 2 <= int(clean.sum()) < len(clean), (k, int(clean.sum()))
        assert not torch.isfinite(raw).all()
