"""The fold of layers_2 into the colour layer (fp16 inference) is admissible by the EXISTING error model, without a GPU.

tests/error_model.py bounds the fp16 kernels by 1.5 x the error of an emulation of the UNFOLDED rounding.  The folded
kernels round other quantities (tests/fold_model.py); this file shows, on the CPU, that the folded emulation itself stays
inside those bounds on every fixture (so the factor 1.5 is still there for what a GPU adds: summation order, ~1 ulp
sines), that it moves PSNR against the teacher by less than the 0.05 dB criterion on the fixture view of each weight set,
and that the folded weights are far inside fp16's range.
"""
import numpy as np
import pytest
import torch

import error_model
import fold_model

KINDS = ("default", "structured")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("kind", KINDS)
def test_folded_mlp_within_the_unfolded_bounds(golden, synthetic, kind):
    g = golden(f"mlp_{kind}.npz")
    sd = synthetic.synthetic_state_dict(0, kind)
    bound, want = error_model.mlp_model(kind, "fp16")
    out = fold_model.forward(sd, t(g["v"])).numpy()
    e_rgb = error_model.scaled_err(out[:, :3], want[:, :3])
    e_sig = error_model.scaled_err(out[:, 3], want[:, 3])
    print(f"mlp {kind}: folded emulation rgb {e_rgb:.3e} (bound {bound['rgb']:.3e}) sigma {e_sig:.3e} (bound {bound['sigma']:.3e})")
    assert e_rgb <= bound["rgb"] and e_sig <= bound["sigma"]
    # sigma never sees the fold: the folded emulation's sigma IS the unfolded one's
    unfolded = error_model.emulated_forward(sd, t(g["v"]), "fp16").numpy()
    assert np.array_equal(out[:, 3], unfolded[:, 3])


@pytest.mark.parametrize("kind", KINDS)
def test_folded_render_within_the_unfolded_bounds(golden, synthetic, kind):
    g = golden(f"render_{kind}.npz")
    sd = synthetic.synthetic_state_dict(0, kind)
    rays = t(g["rays"])
    for N in (32, 64, 128, 192):
        bound, truth = error_model.render_model(kind, "fp16", N)
        outs = fold_model.render(sd, rays, t(g[f"N{N}_u"]))
        ratio = {n: error_model.scaled_err(o.numpy(), truth[n]) / bound[n] for n, o in zip(error_model.NAMES, outs)}
        print(f"render {kind} N={N}: folded emulation error / bound", {k: round(x, 3) for k, x in ratio.items()})
        assert max(ratio.values()) <= 1.0, (N, ratio)


@pytest.mark.parametrize("kind", KINDS)
def test_folded_image_meets_the_psnr_criterion(golden, synthetic, oracle, kind):
    g = golden(f"image_{kind}.npz")
    u = t(golden("image_u.npz")["u"])
    sd = synthetic.synthetic_state_dict(0, kind)
    teacher = synthetic.perturbed_state_dict(sd, seed=1, rel=0.02)
    rays = oracle.camera_rays(t(g["pose"]), [100, 100, synthetic.focal_from_fov(100)])
    cpu = t(g["rgb"])
    with torch.no_grad():
        T, _ = oracle.render_image(teacher, rays, 2500, N=32, u=u)
    img = torch.cat([fold_model.render(sd, rays[s:s + 2500], u[s:s + 2500])[0].clamp(0, 1)
                     for s in range(0, rays.shape[0], 2500)])
    d = float(oracle.img_psnr(T, img)) - float(oracle.img_psnr(T, cpu))
    p_fc = float(oracle.img_psnr(cpu, img))
    p_model, _ = error_model.image_model(kind, "fp16")
    print(f"image {kind}: folded emulation delta PSNR {d:+.4f} dB, PSNR(folded, CPU) {p_fc:.2f} dB (unfolded emulation {p_model:.2f} dB)")
    assert abs(d) <= 0.05
    assert p_fc >= p_model - 1.0          # the allowance test_image_psnr gives the GPU image against the unfolded model


@pytest.mark.parametrize("kind", KINDS)
def test_folded_weights_fit_fp16(synthetic, kind):
    sd = synthetic.synthetic_state_dict(0, kind)
    Wf, bf = fold_model.folded_weights(sd, torch.float64)
    Wf32, bf32 = fold_model.folded_weights(sd)
    assert float(Wf.abs().max()) < 1.0                           # 0.09 / 0.54 against 65504
    # the fp32 fold is not what costs precision: the standard bound of an n-term fp32 dot product, n u sum |a_k b_k|
    # (u = 2^-24, n = 257 with the bias), is orders of magnitude below fp16's 2^-11 relative rounding of the result
    mag = sd["color_fc.0.weight"][:, :256].double().abs() @ sd["layers_2.weight"].double().abs()
    assert bool(((Wf32.double() - Wf).abs() <= 257 * 2.0 ** -24 * mag).all())
    magb = sd["color_fc.0.bias"].double().abs() + sd["color_fc.0.weight"][:, :256].double().abs() @ sd["layers_2.bias"].double().abs()
    assert bool(((bf32.double() - bf).abs() <= 257 * 2.0 ** -24 * magb).all())
