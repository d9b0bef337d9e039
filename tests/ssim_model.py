"""The image metrics' definition in float64 (include/nerf_amd.h) and what fp32 can do with it.

``pred = a`` and ``gt = b`` are [H, W, 3] images with data range 1.

  window      g_k = exp(-(k-5)^2 / (2 1.5^2)), k = 0..10, normalised to sum 1 in double and rounded ONCE to fp32; G_ij = g_i g_j
  position    every (y, x) of [0, H-10) x [0, W-10) and every channel, sums over the 11 x 11 window (no padding):
                  mu_a = sum G a          s_aa = sum G (a - mu_a)^2         s_ab = sum G (a - mu_a)(b - mu_b)
                  ssim_map = (2 mu_a mu_b + C1)(2 s_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(s_aa + s_bb + C2)),  C1 = 0.01^2, C2 = 0.03^2
  image       ssim_c = mean of the map over the positions, ssim = mean of the three channels: tf.image.ssim(max_val=1),
              skimage's structural_similarity(gaussian_weights=True, use_sample_covariance=False, data_range=1)
  the rest    sse_c = sum over all pixels of (a - b)^2, max_gt = max(b); mse = sum_c sse_c / (3 H W), psnr = -10 log10(mse),
              psnr_ref = 20 log10(max_gt) - 10 log10(mse)  (the reference's img_psnr, train.py:21-26: its peak is max(gt))

``ssim_map64`` is that definition.  ``ssim_map32_centred`` evaluates the same centred form in fp32, one rounding per
operation, in the kernel's order (sum G x row by row: sum_i g_i (sum_j g_j x_ij)): the YARDSTICK -- what an fp32 evaluation
of this definition can be held to.  ``ssim_map32_uncentred`` is the usual form, E[a^2] - mu^2 from the same blurs, in fp32:
it cancels, which is why the kernel makes two passes.  ``C_REF_SSIM`` is the yardstick's worst map error over the input
classes and shapes below, in units of 2^-24, measured by ``measure()`` and asserted by tests/test_metrics_cpu.py; the GPU
tests allow 2 C_REF_SSIM + 4 of those units (the project's 2 c + 4 rule)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

WIN, HALO = 11, 10
SIGMA = 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2
EPS = 2.0 ** -24
TILE = 32                                   # csrc/image_metrics.hip T: the edge of a workgroup's tile of positions

# measured by measure(): the centred form's worst class is `smooth` (5.90); the uncentred form on flat white, for the record
# (6.1e-4 of a quantity that lives in [-1, 1])
C_REF_SSIM = 6.0
UNCENTRED_FLAT_WHITE = 10252.0

SHAPES = ((16, 19), (33, 47), (64, 64), (100, 100))
CLASSES = ("noise", "smooth", "flat_white", "step", "near_black", "identical")


def window32():
    k = np.arange(WIN, dtype=np.float64)
    g = np.exp(-(k - 5.0) ** 2 / (2.0 * SIGMA ** 2))
    return (g / g.sum()).astype(np.float32)


def _windows(x):
    """[H, W, 3] -> [H-10, W-10, 3, 11, 11] (a view)."""
    return sliding_window_view(x, (WIN, WIN), axis=(0, 1))


def ssim_map64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    g = window32().astype(np.float64)
    G = np.outer(g, g)
    wa, wb = _windows(a), _windows(b)
    mu_a, mu_b = (wa * G).sum((-2, -1)), (wb * G).sum((-2, -1))
    da, db = wa - mu_a[..., None, None], wb - mu_b[..., None, None]
    s_aa, s_ab, s_bb = (G * da * da).sum((-2, -1)), (G * da * db).sum((-2, -1)), (G * db * db).sum((-2, -1))
    return (2 * mu_a * mu_b + C1) * (2 * s_ab + C2) / ((mu_a ** 2 + mu_b ** 2 + C1) * (s_aa + s_bb + C2))


def metrics64(a, b):
    """The float64 value of everything the library reports, from fp32 images a = pred, b = gt [H, W, >= 3]."""
    a, b = np.asarray(a)[..., :3].astype(np.float64), np.asarray(b)[..., :3].astype(np.float64)
    H, W = a.shape[:2]
    sse = ((a - b) ** 2).sum((0, 1))
    mse = sse.sum() / (3 * H * W)
    out = dict(sse=sse, max_gt=b.max(), mse=mse, psnr=-10 * np.log10(mse) if mse > 0 else np.inf)
    out["psnr_ref"] = 20 * np.log10(out["max_gt"]) + out["psnr"] if out["max_gt"] > 0 else np.nan
    if H >= WIN and W >= WIN:
        out["map"] = ssim_map64(a, b)
        out["ssim_rgb"] = out["map"].mean((0, 1))
        out["ssim"] = out["ssim_rgb"].mean()
    return out


# ---- fp32, one rounding per operation ------------------------------------------------------------------------------------
def _blur32(w, g):
    """sum_i g_i (sum_j g_j w[..., i, j]) in fp32, taps in ascending order: the kernel's order."""
    acc = np.zeros(w.shape[:-2], dtype=np.float32)
    for i in range(WIN):
        h = np.zeros(w.shape[:-2], dtype=np.float32)
        for j in range(WIN):
            h = h + g[j] * w[..., i, j]
        acc = acc + g[i] * h
    return acc


def _quotient32(mu_a, mu_b, s_aa, s_ab, s_bb):
    c1, c2, two = np.float32(C1), np.float32(C2), np.float32(2)
    n1, n2 = two * (mu_a * mu_b) + c1, two * s_ab + c2
    d1, d2 = (mu_a * mu_a + mu_b * mu_b) + c1, (s_aa + s_bb) + c2
    return (n1 * n2) / (d1 * d2)


def ssim_map32_centred(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    g = window32()
    wa, wb = _windows(a), _windows(b)
    mu_a, mu_b = _blur32(wa, g), _blur32(wb, g)
    da, db = wa - mu_a[..., None, None], wb - mu_b[..., None, None]
    assert da.dtype == np.float32
    out = _quotient32(mu_a, mu_b, _blur32(da * da, g), _blur32(da * db, g), _blur32(db * db, g))
    assert out.dtype == np.float32
    return out


def ssim_map32_uncentred(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    g = window32()
    wa, wb = _windows(a), _windows(b)
    mu_a, mu_b = _blur32(wa, g), _blur32(wb, g)
    s_aa = _blur32(wa * wa, g) - mu_a * mu_a
    s_ab = _blur32(wa * wb, g) - mu_a * mu_b
    s_bb = _blur32(wb * wb, g) - mu_b * mu_b
    return _quotient32(mu_a, mu_b, s_aa, s_ab, s_bb)


# ---- the input classes ---------------------------------------------------------------------------------------------------
def images(kind, H, W, seed=0):
    """(pred, gt) fp32 [H, W, 3] in [0, 1] of one class."""
    rng = np.random.default_rng([seed, H, W, CLASSES.index(kind)])
    f32 = np.float32
    if kind == "noise":
        return rng.random((H, W, 3), dtype=f32), rng.random((H, W, 3), dtype=f32)
    if kind == "identical":
        a = rng.random((H, W, 3), dtype=f32)
        return a, a
    if kind == "smooth":
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        a = np.stack([0.5 + 0.4 * np.sin(0.11 * x + 0.07 * y + c) * np.cos(0.05 * y - c) for c in range(3)], -1)
        b = a + 0.05 * np.stack([np.sin(0.23 * x - 0.13 * y + 2 * c) for c in range(3)], -1)
        return a.astype(f32), np.clip(b, 0, 1).astype(f32)
    if kind == "flat_white":                # what background=white produces: 1 with deviations of at most 1 %
        return (1 - 0.01 * rng.random((H, W, 3))).astype(f32), (1 - 0.01 * rng.random((H, W, 3))).astype(f32)
    if kind == "step":                      # black | white, the prediction's edge one pixel off and a little noisy
        a, b = np.zeros((H, W, 3)), np.zeros((H, W, 3))
        b[:, W // 2:] = 1.0
        a[:, W // 2 + 1:] = 1.0
        a = np.clip(a + 0.01 * (rng.random((H, W, 3)) - 0.5), 0, 1)
        return a.astype(f32), b.astype(f32)
    if kind == "near_black":
        return (1e-3 * rng.random((H, W, 3))).astype(f32), (1e-3 * rng.random((H, W, 3))).astype(f32)
    raise ValueError(kind)


def map_error_units(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / EPS)


def measure():
    """{class: (worst centred error, worst uncentred error)} over SHAPES, in units of 2^-24."""
    out = {}
    for kind in CLASSES:
        c = u = 0.0
        for H, W in SHAPES:
            a, b = images(kind, H, W)
            want = ssim_map64(a, b)
            c = max(c, map_error_units(ssim_map32_centred(a, b), want))
            u = max(u, map_error_units(ssim_map32_uncentred(a, b), want))
        out[kind] = (c, u)
    return out


if __name__ == "__main__":
    for kind, (c, u) in measure().items():
        print(f"{kind:12s} centred {c:8.2f}   uncentred {u:10.1f}   (units of 2^-24)")
