"""layers_2 folded into the colour layer of the fp16 inference kernels (csrc/nerf_layout.h, folded view): the packer's
product, the kernels' use of it, its range flag and its following of parameter updates."""
import numpy as np
import pytest
import torch

import error_model
import fold_model
from error_model import TOL

pytestmark = pytest.mark.gpu

KINDS = ("default", "structured")
# the packed 16-bit image (csrc/nerf_layout.h): per layer (16-row tiles, 1 KiB fragments per tile)
TILES_KS = [(16, 2)] + [(16, 8)] * 4 + [(16, 10)] + [(16, 8)] * 2 + [(17, 8), (8, 9), (1, 4)]
L9_OFF_KIB = sum(m * k for m, k in TILES_KS[:9])
WEIGHT_KIB = sum(m * k for m, k in TILES_KS)
L9_BIAS_OFF = sum(m * 16 for m, _ in TILES_KS[:9])
BIAS_FLOATS = sum(m * 16 for m, _ in TILES_KS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with a GPU: pytest -m gpu"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def pack_fp16(flat, dev):
    from nerf_simple_amd import _lib
    lib = _lib.lib()
    packed = torch.empty(lib.nerf_amd_packed_bytes(_lib.FP16), dtype=torch.uint8, device=dev)
    _lib.check(lib.nerf_amd_pack_weights(_lib.ptr(flat), _lib.ptr(packed), _lib.FP16, _lib.stream_ptr(dev)), "pack")
    torch.cuda.synchronize()
    return packed


def colour_layer_of(packed):
    """(W [128, 288 k positions] fp16 as stored, bias [128] fp32, status words) of the packed fp16 image's layer 9."""
    from nerf_simple_amd import _lib
    lib = _lib.lib()
    assert WEIGHT_KIB == 1172 and lib.nerf_amd_packed_status_offset(_lib.FP16) == WEIGHT_KIB * 1024 + BIAS_FLOATS * 4
    raw = packed.cpu().numpy()
    frag = raw[L9_OFF_KIB * 1024:(L9_OFF_KIB + 72) * 1024].view(np.float16).reshape(8, 9, 64, 8)   # [rt][k-step][lane][j]
    W = np.zeros((128, 9, 4, 8), dtype=np.float16)                                                  # [row][k-step][g][j]
    for lane in range(64):
        W[np.arange(8) * 16 + (lane & 15), :, lane >> 4, :] = frag[:, :, lane, :]
    b0 = WEIGHT_KIB * 1024 + L9_BIAS_OFF * 4
    bias = raw[b0:b0 + 128 * 4].view(np.float32).copy()
    status = raw[WEIGHT_KIB * 1024 + BIAS_FLOATS * 4:][:8].view(np.uint32).copy()
    return W, bias, status


def src_cols():
    """source column of the colour layer's weight at (k-step, lane group, element); -1 = padding"""
    from nerf_simple_amd import _lib
    lib = _lib.lib()
    return np.array([[[lib.nerf_amd_layout_src_col(_lib.FP16, 9, s, g, j) for j in range(8)] for g in range(4)]
                     for s in range(9)])


@pytest.mark.parametrize("kind", KINDS)
def test_packed_colour_layer_is_the_folded_product(dev, synthetic, kind):
    sd = synthetic.synthetic_state_dict(0, kind)
    flat = synthetic.flatten_state_dict(sd).to(dev)
    p1, p2 = pack_fp16(flat, dev), pack_fp16(flat, dev)
    assert torch.equal(p1, p2)                                    # a fixed summation order: two packs are bit-equal
    W, bias, status = colour_layer_of(p1)
    assert status[1] == 0
    cols = src_cols()
    assert sorted(cols[:8].ravel()) == list(range(256))           # the chain part: a permutation of h8's 256 features
    Wc, W2 = sd["color_fc.0.weight"].double(), sd["layers_2.weight"].double()
    Wf = (Wc[:, :256] @ W2).numpy()
    want = Wf[:, cols[:8].ravel()].reshape(128, 8, 4, 8)
    got = W[:, :8].astype(np.float64)
    # the packer folds in fp32: its sum is within n u sum |a_k b_k| of the exact product (n = 256, u = 2^-24), so what
    # it stores is the fp16 rounding of SOME value in that interval -- equal to fp16(exact) except next to a rounding
    # boundary, and then one fp16 ulp away
    slack = (256 * 2.0 ** -24 * (Wc[:, :256].abs() @ W2.abs()).numpy())[:, cols[:8].ravel()].reshape(128, 8, 4, 8)
    lo, hi = (want - slack).astype(np.float16).astype(np.float64), (want + slack).astype(np.float16).astype(np.float64)
    assert np.all((got >= lo) & (got <= hi))
    nearest = want.astype(np.float16)
    ulp = np.spacing(np.abs(nearest)).astype(np.float64)
    off = np.abs(got - nearest.astype(np.float64))
    print(f"{kind}: folded fragments differing from fp16(float64 product): {int((off > 0).sum())} of {off.size}, max |Wf| {np.abs(Wf).max():.3f}")
    assert np.all(off <= ulp)
    assert (off > 0).mean() <= 0.01                               # boundary cases only
    # the direction part is the plain weight, padding is zero
    dcols = cols[8]
    plain = np.where(dcols[None] >= 0, sd["color_fc.0.weight"].numpy()[:, np.maximum(dcols, 0).ravel()].reshape(128, 4, 8), 0.0)
    assert np.array_equal(W[:, 8], plain.astype(np.float16))
    # bias: bc + Wc[:, :256] b2
    bf = (sd["color_fc.0.bias"].double() + Wc[:, :256] @ sd["layers_2.bias"].double()).numpy()
    err = float(np.abs(bias.astype(np.float64) - bf).max())
    print(f"{kind}: folded bias max error {err:.3e} (bound {error_model.ULP_FLOOR * max(1.0, float(np.abs(bf).max())):.3e})")
    assert err <= error_model.ULP_FLOOR * max(1.0, float(np.abs(bf).max()))


@pytest.mark.parametrize("kind", KINDS)
def test_fp16_forward_is_the_folded_emulation(dev, golden, synthetic, kind):
    """Attribution: the fp16 kernel sits at least as close to the emulation of ITS numerics (tests/fold_model.py) as to
    the fp32 golden; a wrong fold shows here before it shows in a tolerance."""
    from nerf_simple_amd.utils.nets import Nerf
    g = golden(f"mlp_{kind}.npz")
    sd = synthetic.synthetic_state_dict(0, kind)
    net = Nerf(precision="fp16").to(dev)
    net.load_state_dict(sd)
    with torch.no_grad():
        out = net(t(g["v"]).to(dev)).cpu().numpy()
    emu = fold_model.forward(sd, t(g["v"])).numpy()
    for name, sl in (("rgb", slice(0, 3)), ("sigma", 3)):
        e_emu = error_model.scaled_err(out[:, sl], emu[:, sl])
        e_gold = error_model.scaled_err(out[:, sl], g["out"][:, sl])
        print(f"mlp {kind} fp16 {name}: against the folded emulation {e_emu:.3e}, against the golden {e_gold:.3e}")
        assert e_emu <= e_gold


def test_folded_product_beyond_fp16_is_flagged_at_pack(dev, synthetic):
    """Factors that fit fp16 whose product does not: flagged like an unfittable plain weight, demoted to bf16."""
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils.nets import Nerf, packed_status
    sd = {k: v.clone() for k, v in synthetic.synthetic_state_dict(0, "default").items()}
    # max |Wf| of the default set is 0.09: a gain of 2000 on each factor puts it at 3.6e5
    sd["layers_2.weight"] *= 2000.0
    sd["color_fc.0.weight"][:, :256] *= 2000.0
    assert all(float(v.abs().max()) < 65504 / 4 for v in sd.values())                     # every factor fits
    Wf, _ = fold_model.folded_weights(sd, torch.float64)
    assert float(Wf.abs().max()) > 2 * 65504                                               # the product does not
    net = Nerf().to(dev)
    assert net.precision == "fp16"
    net.load_state_dict(sd)
    assert packed_status(net.packed_weights(_lib.FP16), _lib.FP16) == _lib.STATUS_WEIGHT_RANGE
    assert packed_status(net.packed_weights(_lib.BF16), _lib.BF16) == 0
    v = synthetic.points_in_scene(64, seed=2).to(dev)
    with torch.no_grad():
        with pytest.warns(UserWarning, match="a weight beyond 65504"):
            out = net(v)
        assert torch.equal(out, net(v, precision="bf16"))


@pytest.mark.parametrize("kind", KINDS)
def test_folded_image_follows_layers_2_updates(dev, oracle, synthetic, kind):
    from nerf_simple_amd.utils.nets import Nerf
    sd = synthetic.synthetic_state_dict(0, kind)
    net = Nerf(precision="fp16").to(dev)
    net.load_state_dict(sd)
    v = synthetic.points_in_scene(256, seed=4)
    tol = TOL[("fp16", kind)]
    with torch.no_grad():
        before = oracle.nerf_forward(sd, v).numpy()
        a = net(v.to(dev)).cpu().numpy()
        assert error_model.scaled_err(a, before) <= tol
        net.layers_2.bias.add_(0.25)
        net.layers_2.weight[3, 5] += 0.5
        sd2 = {k: p.detach().cpu().clone() for k, p in net.state_dict().items()}
        b = net(v.to(dev)).cpu().numpy()
        after = oracle.nerf_forward(sd2, v).numpy()
    moved = error_model.scaled_err(after, before)
    err = error_model.scaled_err(b, after)
    print(f"{kind}: the update moves the output by {moved:.3e} (scaled); fp16 against the oracle on the new weights {err:.3e} (tol {tol:.3e})")
    assert moved > 4 * tol                                        # a stale image would not pass
    assert err <= tol
    assert np.array_equal(b[:, 3], a[:, 3])                      # sigma does not see layers_2
