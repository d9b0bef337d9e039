"""The training controls -- a background colour, sigma noise, the distortion loss -- stated once (DESIGN.md section 37 holds
the table of entry point x term x keyword x refusal; tests/test_controls_rule_cpu.py walks it).  A leaf: ``_lib`` and torch.

Three things live here.  ``Controls``: what a caller passes (or the flat keywords that mean the same).  ``Resolved``: what
everything below an entry point's preamble receives -- the background as the kernels take it, the noise's key, the term's
weight; ``None`` where nothing is on, so a call without controls is the call it was.  The rules: each refusal's sentence
once, raised before any launch, any RNG draw and any ``optimizer.zero_grad``.
"""
import math
from typing import NamedTuple, Optional

import torch

from .. import _lib

# The coarse + fine pair: both passes draw their sigma noise with ``controls.sigma_noise``, the coarse one
# under ``noise_seed``, the fine one under (noise_seed + FINE_NOISE_OFFSET) mod 2^64.  The noise counter is (ray_id0 + ray) N + i
# with N = Nc or Nc + Nf: under ONE key the two passes would share words across different rays.  A graphed stepper adds its step
# count to the seed, which never crosses 2^63.
FINE_NOISE_OFFSET = 1 << 63


def _finite_nonneg(x, what):
    v = float(x)
    if not (v >= 0.0) or math.isinf(v):
        raise ValueError(f"{what}: finite and >= 0, got {x!r}")
    return v


def _refuse_with(paths, message):
    """``paths`` = {what: value}: the first one that is set refuses, under its name."""
    for name, v in paths.items():
        if v is not None:
            raise RuntimeError(message.format(name))


def check_distortion(distortion, paths=None):
    """The flat ``distortion=`` as a weight: a finite float >= 0 (0 = off), else ValueError.  ``paths``: the masked, hierarchical
    and sharded paths this entry point has ({what: value}); they do not take the flat keyword (RuntimeError)."""
    lam = _finite_nonneg(distortion, "distortion is the weight of the distortion loss")
    if lam and paths:
        _refuse_with(paths, "distortion serves the dense and guided steps only: not with {} (train without the term, or on the "
                            "dense path)")
    return lam


def background_shape(n, shape):
    """The background's shape rule, for a table of ``n`` rays."""
    return RuntimeError(f"background must be one colour [3] or one per ray [{n}, 3], got {tuple(shape)}")


def background_arg(background, B, dev):
    """``background`` as the kernels take it: (fp32 contiguous tensor on ``dev``, stride) -- one colour [3] (stride 0) or one
    per ray [B,3] (stride 3).  A sequence of three numbers is a colour.  It carries no gradient."""
    if not torch.is_tensor(background):
        background = torch.tensor([float(x) for x in background], dtype=torch.float32)
    bg = background.detach().to(device=dev, dtype=torch.float32).contiguous()
    if tuple(bg.shape) == (3,):
        return bg, 0
    if tuple(bg.shape) == (B, 3):
        return bg, 3
    raise background_shape(B, bg.shape)


class Controls:
    """``Controls(background=None, sigma_noise=0.0, noise_seed=0, distortion=0.0)``: the training controls as one frozen value --
    a background colour ([3], or one per ray [B,3]) behind the volume, the standard deviation of Gaussian noise on the raw
    density with the counter RNG's ``noise_seed``, and the weight of the distortion loss (``train_step`` describes each).
    Validated here as the flat keywords are (ValueError for a negative or non-finite ``sigma_noise`` / ``distortion``); the
    background's shape is checked where the number of rays is known.  ``controls=`` is the one keyword the masked steps take
    them through; on the dense steps it is the equivalent of the flat keywords, so a grid can be toggled without respelling
    the call."""

    __slots__ = ("background", "sigma_noise", "noise_seed", "distortion")

    def __init__(self, background=None, sigma_noise=0.0, noise_seed=0, distortion=0.0):
        set_ = object.__setattr__
        set_(self, "background", background)
        set_(self, "sigma_noise", _finite_nonneg(sigma_noise, "sigma_noise is a standard deviation"))
        set_(self, "noise_seed", int(noise_seed))
        set_(self, "distortion", check_distortion(distortion))

    def __setattr__(self, name, value=None):
        raise AttributeError(f"Controls is frozen: build a new one to change {name!r}")

    __delattr__ = __setattr__

    def __repr__(self):
        return (f"Controls(background={self.background!r}, sigma_noise={self.sigma_noise!r}, noise_seed={self.noise_seed!r}, "
                f"distortion={self.distortion!r})")

    def replace(self, **changes):
        """A new Controls with some fields changed."""
        return Controls(**{**{n: getattr(self, n) for n in self.__slots__}, **changes})


class Resolved(NamedTuple):
    """A Controls once the batch is known: what the renders, the compositor and the steppers receive."""
    bg: Optional[torch.Tensor]      # fp32 [3] or [B,3] on the device, or None
    stride: int                     # 0: one colour, 3: one per ray
    std: float                      # sigma noise's standard deviation, 0.0 = off
    noise_seed: int
    noise_ray_id0: int              # global id of the first ray, as the noise counter takes it
    lam: float                      # the distortion term's weight, 0.0 = off

    def fine(self):
        """The fine pass of a coarse + fine pair: the same record under its own noise key."""
        return self._replace(noise_seed=(self.noise_seed + FINE_NOISE_OFFSET) % (1 << 64))


def resolve(c, B, dev, ray_id0=0):
    """A Controls (or None) -> its Resolved for ``B`` rays on ``dev``, or None where nothing is on.  The background's shape is
    looked at here (RuntimeError)."""
    if c is None or (c.background is None and not c.sigma_noise and not c.distortion):
        return None
    bg = (None, 0) if c.background is None else background_arg(c.background, B, dev)
    return Resolved(*bg, c.sigma_noise, c.noise_seed, int(ray_id0), c.distortion)


# ---- the rules: one statement each ----------------------------------------------------------------------------------------------
def bundle(controls, *, background=None, sigma_noise=0.0, noise_seed=0, distortion=0.0):
    """``controls=`` of an entry point: None, or a Controls -- TypeError for anything else, ValueError where the flat keywords of
    the same call (passed on here by those entry points that have them) say something too."""
    if controls is None:
        return None
    if not isinstance(controls, Controls):
        raise TypeError(f"controls must be a training.Controls (or None), got {type(controls).__name__}")
    if background is not None or sigma_noise or noise_seed or distortion:
        raise ValueError("controls= and the flat keywords background / sigma_noise / noise_seed / distortion say the same thing: "
                         "give one of the two")
    return controls


def from_keywords(controls, paths, *, background=None, sigma_noise=0.0, noise_seed=0, distortion=0.0):
    """``controls=`` or the flat keywords of an entry point that has both -> a Controls, or None where neither says anything.
    In order: ``bundle``; then, for the flat keywords, the weight's ValueError and the two dense-only refusals under ``paths``;
    the noise's ValueError comes last."""
    c = bundle(controls, background=background, sigma_noise=sigma_noise, noise_seed=noise_seed, distortion=distortion)
    if c is not None:
        return c
    lam = check_distortion(distortion, paths)
    if background is not None or sigma_noise:          # the flat pair knows the dense path alone
        _refuse_with(paths, "background / sigma_noise serve the dense path only: not with {}= (render without them, or without "
                            "the grid)")
    if background is None and not sigma_noise and not lam:
        return None                           # off by default: a call without them is the call it was
    return Controls(background, sigma_noise, noise_seed, lam)


def render_only(c, terminate=None, hint=""):
    """What a render (as opposed to a step) takes of a bundle: not with ``terminate=``, and no distortion term."""
    if c is None:
        return
    if terminate is not None:
        raise RuntimeError("controls= does not reach the terminated render yet: not with terminate=")
    if c.distortion:
        raise ValueError(f"the distortion term belongs to a training step{hint}: a render takes controls.distortion == 0")


def refuse_noise(tail):
    """Sigma noise where nothing trains.  ``tail``: what the entry point says about itself."""
    raise RuntimeError(f"sigma_noise is a training regulariser, not a render option: {tail}")


def pair(controls, what):
    """``controls=`` of a coarse + fine entry point, the FIRST thing it looks at: None, or a Controls (TypeError) whose
    distortion term is off (RuntimeError, before any look at the networks, the optimiser, the grid or the generator) -- the
    regulariser belongs on the final weights, not on what places the samples.  -> the Controls, or None where nothing is on;
    the coarse pass takes its ``resolve``, the fine pass that record's ``fine()``."""
    controls = bundle(controls)
    if controls is None:
        return None
    if controls.distortion > 0:
        raise RuntimeError(f"controls= brings the background and the sigma noise to {what}: the distortion term "
                           "(controls.distortion) is not offered on the coarse + fine pair")
    if controls.background is None and not controls.sigma_noise:
        return None
    return controls


def refuse_bundle(controls, what):
    """The paths ``controls=`` does not reach yet: refused before any launch and any RNG draw."""
    if controls is not None:
        bundle(controls)
        raise RuntimeError(f"controls= serves the dense and the masked single-network steps: not {what}")


def refuse_flat(what, background=None, sigma_noise=0.0, distortion=0.0):
    """The steppers that know none of the three terms (the camera and appearance steppers)."""
    if background is not None or sigma_noise or distortion:
        raise RuntimeError(f"{what} does not take background / sigma_noise / distortion yet")


# ---- the blend: the one launch behind the background ---------------------------------------------------------------------------
def blend(rgb, acc, disp, bg, stride, pixels=False):
    """rgb + (1 - acc) bg through nerf_amd_background_blend: rgb_bg [B,3], or pixels [B,4] = [clip(rgb_bg, 0, 1), disp]."""
    B, dev = rgb.shape[0], rgb.device
    out = torch.empty((B, 4 if pixels else 3), dtype=torch.float32, device=dev)
    _lib.launch("nerf_amd_background_blend", rgb, acc, disp if pixels else None, bg, stride, None if pixels else out,
                out if pixels else None, B, dev=dev)
    return out


def blended(out, c, pixels=False):
    """An inference render's 5-tuple behind the background of ``c`` (a Resolved; None or one without a background: ``out`` as it
    is): rgb blended, the other four as they were; ``pixels=True``: [clip(rgb_bg, 0, 1), disp] [B,4] instead."""
    if c is None or c.bg is None:
        return out
    if pixels:
        return blend(out[0], out[3], out[1], c.bg, c.stride, pixels=True)
    return (blend(out[0], out[3], None, c.bg, c.stride),) + tuple(out[1:])


class Background(torch.autograd.Function):
    """(rgb [B,3], acc [B]) -> rgb_bg = rgb + (1 - acc) bg (nerf_amd_background_blend); backward: g_rgb passes through,
    g_acc from nerf_amd_background_blend_backward -- autograd adds it to whatever else reaches acc, and the sum enters
    the compositor's backward, which already takes g_acc.  ``bg`` [3] (stride 0) or [B,3] (stride 3) carries no gradient."""

    @staticmethod
    def forward(ctx, rgb, acc, bg, stride):
        rgb, acc = rgb.contiguous(), acc.contiguous()
        ctx.save_for_backward(bg)
        ctx.stride = stride
        return blend(rgb, acc, None, bg, stride)

    @staticmethod
    def backward(ctx, g):
        (bg,) = ctx.saved_tensors
        g = g.contiguous().float()
        B, dev = g.shape[0], g.device
        g_acc = torch.empty((B,), dtype=torch.float32, device=dev)
        _lib.launch("nerf_amd_background_blend_backward", g, bg, ctx.stride, g_acc, B, dev=dev)
        return g, g_acc, None, None
