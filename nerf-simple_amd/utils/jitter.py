"""The jitter source rule of the eager entry points, stated once (DESIGN.md section 31 holds the table of entry point x
jitter arguments; tests/test_jitter_rule_cpu.py walks it).  ``host_rng`` is the generator; this is what sits on top.

Precedence: explicit positions ``ts`` (FLAG_TS_GIVEN) > explicit uniforms ``u`` (flags 0) > ``device_rng`` (FLAG_DEVICE_RNG,
no tensor) > one ``torch.rand(B, N)`` of torch's CPU generator, continued on the device (``host_rng.reference_rand``).
Nothing here raises after a draw: a refused call leaves the generator where it was.
"""
import torch

from .. import _lib
from . import host_rng

_tbins_cache = {}
SHAPE_ERROR = "u / ts must be [B, N]"       # render_nerf's, OccupancyGrid.mark's and render_nerf_masked's message


def check(B, N, *, u=None, ts=None, names=("u", "ts"), shape_error=SHAPE_ERROR):
    """A given ``ts`` / ``u`` is float32 on the GPU and [B, N].  ``shape_error``: the entry point's message for another
    shape; None: this entry point does not look at the shape here (section 31 says where it does)."""
    for name, t_ in ((names[1], ts), (names[0], u)):
        if t_ is None:
            continue
        _lib.require_cuda_f32(t_, name)
        if shape_error is not None and tuple(t_.shape) != (B, N):
            raise RuntimeError(shape_error)


def single(B, N, dev, *, u=None, ts=None, device_rng=False, names=("u", "ts"), shape_error=SHAPE_ERROR):
    """One jitter argument set -> (jitter tensor or None, flags, pending generator session or None): ``check`` first, then
    the precedence.  ``pending`` is not finished: the caller calls ``.finish()`` once what follows the draw is enqueued
    (or at once)."""
    check(B, N, u=u, ts=ts, names=names, shape_error=shape_error)
    if ts is not None:
        return ts.contiguous(), _lib.FLAG_TS_GIVEN, None
    if u is not None:
        return u.contiguous(), 0, None
    if device_rng:
        return None, _lib.FLAG_DEVICE_RNG, None
    # the reference's single CPU draw per call (utils/rendering.py:28-30): same numbers, same advance of torch's CPU
    # generator, produced on the device
    jit, pending = host_rng.reference_rand(B, N, dev)
    return jit, 0, pending


def pair(B, Nc, Nf, dev, *, u_c=None, u_f=None, device_rng=False):
    """The coarse / fine pair -> (coarse jitter or None, coarse flags, u_f or None): a given ``u_c`` wins over
    ``device_rng``; the draws run ``u_c`` then ``u_f``, each finished at once; ``u_f`` is drawn only when it is absent and
    ``device_rng`` is off (the fine sampler then takes the counter RNG)."""
    _lib.require_shape(u_c, "u_c", (B, Nc))
    _lib.require_shape(u_f, "u_f", (B, Nf))
    jit_c, flags_c, pending = single(B, Nc, dev, u=u_c, device_rng=device_rng, shape_error=None)
    if pending is not None:
        pending.finish()
    u_f, _, pending = single(B, Nf, dev, u=u_f, device_rng=device_rng, shape_error=None)
    if pending is not None:
        pending.finish()
    return jit_c, flags_c, u_f


def tbins(tn, tf, N, device, flags=0):
    """The bin edges the kernels jitter in (one cached tensor per interval, count and device), or None when the positions are
    given."""
    if flags & _lib.FLAG_TS_GIVEN:
        return None
    key = (float(tn), float(tf), int(N), device)
    t = _tbins_cache.get(key)
    if t is None:
        # computed on the host by torch.linspace so bin edges are bit-identical
        # to the reference's (utils/rendering.py:25)
        t = torch.linspace(tn, tf, N + 1).to(device)
        if len(_tbins_cache) > 64:
            _tbins_cache.clear()
        _tbins_cache[key] = t
    return t
