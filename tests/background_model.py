"""CPU model of the dense path's two training controls (test infrastructure; uses the oracle): the sigma-noise regulariser
(csrc/sigma_noise_device.h) and the background blend (csrc/composite_bg.hip), and the float64 value of the head that carries
both (nerf_amd_volume_render_mse_backward_bg).  Imports oracle.nerf_oracle.philox_word and tests/ray_routines_model.py and
edits neither.

Noise.  Sample s = (ray_id0 + ray) N + i owns the counters 2 s and 2 s + 1 under the key (noise_seed + offset) ^ NOISE_KEY:
    u1 = ((word(2 s) >> 8) + 1) 2^-24 in (0, 1],  u2 = (word(2 s + 1) >> 8) 2^-24 in [0, 1)       (both exact in fp32)
    r = sqrt(-2 ln u1),  z = r cos(2 pi u2)
evaluated here in float64 on the oracle's words.

K_NOISE: the routine's fp32 z against that value, |z_fp32 - z| <= K_NOISE EPS (1 + r), EPS = 2^-24, derived from the documented
accuracy of the functions the routine calls (HIP's device math functions: logf, sqrtf, cospif each within 1 ulp; 1 ulp of x is
at most 2 EPS |x|) and one rounding (EPS relative) per explicitly rounded product:
    L^ = logf(u1)                    |L^ - L| <= 2 EPS |L|                      (u1 exact; -2 L^ exact)
    r^ = sqrtf(-2 L^)                sqrt halves the relative error: EPS, + its own 1 ulp = 2 EPS  ->  |r^ - r| <= 3 EPS r
    c^ = cospif(2 u2)                2 u2 exact; |c^ - c| <= 2 EPS |c| <= 2 EPS
    z^ = fl(r^ c^)                   |z^ - r c| <= r |c^ - c| + |c| |r^ - r| + EPS |z| <= (2 + 3 + 1) EPS r = 6 EPS r
With the error model's usual margin of 1.5: K_NOISE = 9.  (std = 1 on sigma = 0 adds nothing: 1 z and 0 + z are exact.)
Nothing here is taken from what a GPU shows.

Blend.  rgb_bg = rgb + (1 - acc) bg and g_acc = -((g0 bg0 + g1 bg1) + g2 bg2) as separately rounded torch fp32 ops: the
kernels' definition, compared with torch.equal.

Head against float64.  loss = MSE(rgb + (1 - acc) bg, gt) on sigma' (the kernel's own noise, read back): its gradient is the
compositor's backward with the upstream gradients g_rgb = 2 (rgb_bg - gt) / (3 B), g_acc = -g_rgb . bg, both from the float64
forward; ray_routines_model.model_backward gives the value and the first-order bound A, ray_routines_model.ray_ratios the
two ratios per ray.  The existing constants C_REF_RAY['all'] / C_REF_RAY_PLAIN['all'] were measured with upstream gradients
that are GIVEN; here they are formed from the forward in fp32 as well (rgb_bg - gt carries the forward's rounding into
every element), so this upstream has constants of its own, C_REF_BG / C_REF_BG_PLAIN: the largest ratio of the reference's
own fp32 evaluation (oracle.volume_render + the blend + MSE under fp32 autograd) over head_cases() in every mode, written by

    python tests/background_model.py            (a minute on a CPU; prints the two constants)

rounded up to two digits; tests/test_background_cpu.py asserts that the oracle's fp32 evaluation stays inside them, and the
GPU test allows the model's usual  bound(c) = 2 c + 4.
"""
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "oracle"), os.path.join(_ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import nerf_oracle as O  # noqa: E402
import ray_routines_model as M  # noqa: E402

EPS = M.EPS
NOISE_KEY = 0x6e6f6973653a7631          # csrc/sample_pdf_device.h NOISE_KEY ("noise:v1")
RNG_KEY = 0x9e3779b97f4a7c15            # csrc/sample_pdf_device.h RNG_KEY, the sampler's
SELECT_KEY = O.SELECT_KEY               # the ray selection's
K_NOISE = 9.0                           # derived in the module docstring
_M64 = 0xffffffffffffffff

# measured on the CPU by `python tests/background_model.py` (see the module docstring)
C_REF_BG = 2.9
C_REF_BG_PLAIN = 19.0


# ---- noise ------------------------------------------------------------------------------------------------------------------
def noise_key(noise_seed, offset=0):
    return ((int(noise_seed) + int(offset)) & _M64) ^ NOISE_KEY


def noise_uniforms(noise_seed, ray_id0, B, N, offset=0):
    """(u1, u2) [B,N] float64 of the samples of rays ray_id0 .. ray_id0 + B."""
    s = (np.uint64(ray_id0) * np.uint64(N) + np.arange(B * N, dtype=np.uint64)).reshape(B, N)
    key = noise_key(noise_seed, offset)
    w1, w2 = O.philox_word(key, np.uint64(2) * s), O.philox_word(key, np.uint64(2) * s + np.uint64(1))
    return ((w1 >> np.uint32(8)).astype(np.float64) + 1.0) * EPS, (w2 >> np.uint32(8)).astype(np.float64) * EPS


def noise_normal(noise_seed, ray_id0, B, N, offset=0):
    """(z, r) [B,N] float64: the Box-Muller normal of every sample and its radius sqrt(-2 ln u1)."""
    u1, u2 = noise_uniforms(noise_seed, ray_id0, B, N, offset)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r


def noise_bound(r):
    return K_NOISE * EPS * (1.0 + r)


def jitter_uniforms(seed, ray_id0, B, N):
    """The stratified jitter of the same samples under the counter RNG (csrc/nerf_device.h: key = the bare seed)."""
    s = (np.uint64(ray_id0) * np.uint64(N) + np.arange(B * N, dtype=np.uint64)).reshape(B, N)
    return (O.philox_word(int(seed) & _M64, s) >> np.uint32(8)).astype(np.float64) * EPS


# ---- blend ------------------------------------------------------------------------------------------------------------------
def blend(rgb, acc, bg):
    """rgb [B,3], acc [B], bg [3] or [B,3] -> rgb_bg: three separately rounded fp32 torch ops."""
    return rgb + (1 - acc)[:, None] * bg


def blend_backward(g, bg):
    """g [B,3] -> g_acc [B] = -((g0 bg0 + g1 bg1) + g2 bg2), every product and sum rounded on its own, in that order."""
    b = bg.expand_as(g)
    return -((g[:, 0] * b[:, 0] + g[:, 1] * b[:, 1]) + g[:, 2] * b[:, 2])


def pixels(rgb_bg, disp):
    return torch.cat([torch.clip(rgb_bg, 0., 1.), disp[:, None]], dim=1)


def mse_gradient(rgb, target):
    """The MSE head's g = 2 (rgb - target) / (3 B) as the kernels form it (csrc/composite_backward_device.h)."""
    B = rgb.shape[0]
    scale = (torch.tensor(1.0) / (torch.tensor(3.0) * torch.tensor(float(B)))).to(rgb.device)
    return 2.0 * (rgb - target) * scale


# ---- the head's cases -------------------------------------------------------------------------------------------------------
HEAD_N = (2, 63, 64, 65, 128, 129, 512)
MODES = ("bg1", "bgB", "noise", "both", "neither")       # background [3] / [B,3], noise alone, both (per ray), neither
NOISE_STD = 0.75


def head_cases():
    """ray_routines_model.comp_cases() at the chunk seams: every density set at every N, B cycling through 1, 5, 37."""
    return [c for c in M.comp_cases() if c.N in HEAD_N]


def head_inputs(case):
    """raw, ts, rays [B,6] (comp_inputs' directions behind random origins), target [B,3] in [0,1], bg1 [3], bgB [B,3]."""
    raw, ts, d = M.comp_inputs(case)
    g = torch.Generator().manual_seed(case.seed + 31)
    B = case.B
    rays = torch.cat([torch.randn(B, 3, generator=g), d], dim=1)
    return raw, ts, rays, torch.rand(B, 3, generator=g), torch.rand(3, generator=g), torch.rand(B, 3, generator=g)


def unit_dirs(rays):
    """rays[:, 3:] / ||rays[:, 3:]|| in fp32: the kernels' own normalisation (and render_nerf's, utils/rendering.py:37)."""
    d = rays[:, 3:]
    return d / torch.norm(d, dim=1, keepdim=True)


def mode_controls(mode, bg1, bgB):
    """(bg or None, std) of a mode."""
    return {"bg1": (bg1, 0.0), "bgB": (bgB, 0.0), "noise": (None, NOISE_STD), "both": (bgB, NOISE_STD), "neither": (None, 0.0)}[mode]


def head_model(raw_noisy, ts, rays, target, bg):
    """float64 (want [B,N,4], A [B,N,4], rgb_bg [B,3]) of d MSE(rgb + (1 - acc) bg, target) / d raw on the noisy raw."""
    dn = unit_dirs(rays)
    fw = M.forward64(raw_noisy, ts, dn)
    B = ts.shape[0]
    rgb = (fw["w"][..., None] * raw_noisy[..., :3].double()).sum(dim=1)
    acc = fw["w"].sum(dim=1)
    b = torch.zeros(B, 3, dtype=torch.float64) if bg is None else bg.double().expand(B, 3)
    rgb_bg = rgb + (1 - acc)[:, None] * b
    g_rgb = 2.0 * (rgb_bg - target.double()) / (3.0 * B)
    g_acc = None if bg is None else -(g_rgb * b).sum(dim=1)
    want, A = M.model_backward(fw, raw_noisy, ts, [g_rgb, None, None, g_acc, None])
    return want, A, rgb_bg.numpy()


def oracle_head_grad(raw_noisy, ts, rays, target, bg, dtype):
    """The same gradient through the oracle's autograd in ``dtype`` (the reference's own evaluation), float64 numpy."""
    r = raw_noisy.to(dtype).clone().requires_grad_(True)
    rgb, _, _, acc, _ = O.volume_render(r, ts.to(dtype), unit_dirs(rays).to(dtype))
    if bg is not None:
        rgb = rgb + (1 - acc)[:, None] * bg.to(dtype)
    torch.mean((rgb - target.to(dtype)) ** 2).backward()
    return r.grad.double().numpy()


def cpu_noisy(raw, std, noise_seed, N):
    """raw with the float64 model's noise, rounded to fp32: the CPU stand-in for the kernel's own noise."""
    z, _ = noise_normal(noise_seed, 0, raw.shape[0], N)
    out = raw.clone()
    out[..., 3] = (raw[..., 3].double() + std * torch.from_numpy(z)).float()
    return out


def measure():
    c_cond = c_plain = 0.0
    for case in head_cases():
        raw, ts, rays, target, bg1, bgB = head_inputs(case)
        for mode in MODES:
            bg, std = mode_controls(mode, bg1, bgB)
            rn = cpu_noisy(raw, std, case.seed, case.N) if std else raw
            want, A, _ = head_model(rn, ts, rays, target, bg)
            ref32 = oracle_head_grad(rn, ts, rays, target, bg, torch.float32)
            cond, plain = M.ray_ratios(ref32, want, A, np.isfinite(ref32))
            c_cond, c_plain = max(c_cond, float(cond.max())), max(c_plain, float(np.nanmax(plain, initial=0.0)))
    return c_cond, c_plain


if __name__ == "__main__":
    print("C_REF_BG = %.3g   C_REF_BG_PLAIN = %.3g" % measure())
