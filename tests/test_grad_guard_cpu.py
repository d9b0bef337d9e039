"""The gradient guard without a GPU: the ``max_grad_norm`` argument rule, the numpy model of the
definition (tests/grad_guard_model.py) against ``torch.nn.utils.clip_grad_norm_`` on CPU tensors, and the three entry points
in the header, in the binding's table and refusing bad arguments before anything is launched."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import grad_guard_model as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nerf_amd_grad_guard_workspace_bytes", "nerf_amd_grad_guard", "nerf_amd_adam_step_guarded")


@pytest.mark.parametrize("bad", [float("nan"), 0, 0.0, -1.0, -float("inf"), "1.0", [1.0], True, 1 + 0j])
def test_max_grad_norm_is_checked_before_the_device(bad):
    from nerf_simple_amd.optim import FusedAdam, check_max_grad_norm
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam(torch.nn.Linear(2, 2), max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        check_max_grad_norm(bad)


@pytest.mark.parametrize("good", [None, 1, 0.5, 1e-30, float("inf")])
def test_a_valid_max_grad_norm_reaches_the_device_check(good):
    """A valid limit passes the argument rule: a CPU module is then refused for what it is, as it always was."""
    from nerf_simple_amd.optim import FusedAdam, check_max_grad_norm
    with pytest.raises(RuntimeError, match="needs the module on the GPU"):
        FusedAdam(torch.nn.Linear(2, 2), max_grad_norm=good)
    if good is not None:
        assert check_max_grad_norm(good) == float(good) and isinstance(check_max_grad_norm(good), float)


def _ulps(a, b):
    """The distance of two fp32 arrays in units in the last place (ordered-integer distance)."""
    def key(x):
        i = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("scale, max_norm", [(1.0, 0.5), (1.0, 1e3), (1e-3, 1.0), (30.0, 2.0), (1.0, float("inf"))])
def test_model_is_clip_grad_norm(scale, max_norm):
    """torch forms the norm in fp32 (a norm per tensor, then the norm of those): for these 1,391 elements its error is a few
    units of 2^-24 -- each of its two fp32 reductions sums at most 1,024 terms in a vectorised / pairwise order whose error
    bound is about log2(1024) = 10 roundings, and the square root halves a relative error: 16 ulp holds all of it -- while
    the model's norm is the correctly rounded one.  Given the SAME norm the model's coef is torch's clamp(max_norm / (norm +
    1e-6), max=1) operation for operation, so the clipped gradients are the same fp32 products: within 1 ulp (0 expected)."""
    gen = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter(torch.zeros(s)) for s in ((32, 32), (7, 51), (10,))]
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen) * scale
    flat = torch.cat([p.grad.reshape(-1) for p in params]).numpy().copy()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    want = G.norm32(flat)
    assert not G.skip(want)
    assert abs(float(total) - float(want)) <= 16 * G.ulp(want), (float(total), float(want))
    c = G.coef(max_norm, np.float32(float(total)))
    assert c.dtype == np.float32 and 0 < c <= 1 and (c < 1) == (float(total) + 1e-6 > max_norm)
    clipped = torch.cat([p.grad.reshape(-1) for p in params]).numpy()
    mine = flat if c == 1 else flat * c
    assert mine.dtype == np.float32 and _ulps(mine, clipped).max() <= 1
    if math.isinf(max_norm):
        assert c == 1 and np.array_equal(clipped, flat)


def test_model_skip_rule_and_ranges():
    """The double sum neither overflows nor underflows on finite fp32 gradients; the skip rule is the norm's, so a finite
    gradient whose norm leaves the fp32 range skips too."""
    n = 595844
    assert G.norm64(np.full(n, 3e19, np.float32)) == pytest.approx(3e19 * math.sqrt(n), rel=1e-6) and not G.skip(G.norm32(np.full(n, 3e19, np.float32)))
    tiny = G.norm32(np.full(n, 1e-30, np.float32))
    assert tiny > 0 and float(tiny) == pytest.approx(1e-30 * math.sqrt(n), rel=1e-6)
    assert G.skip(G.norm32(np.full(n, 3e38, np.float32))) and G.coef(1.0, G.norm32(np.full(n, 3e38, np.float32))) == 0
    for bad in (np.nan, np.inf, -np.inf):
        g = np.ones(5, np.float32)
        g[3] = bad
        assert G.skip(G.norm32(g)) and G.coef(1.0, G.norm32(g)) == 0
    assert G.norm32(np.zeros(0, np.float32)) == 0 and G.coef(1.0, np.float32(0)) == 1 and not G.skip(np.float32(0))
    assert G.coef(float("inf"), np.float32(3e38)) == 1
    # each operation rounded on its own: 1 / (1 + 1e-6) in fp32 is below 1 although 1 + 1e-6 rounds to the next fp32
    assert G.coef(1.0, np.float32(1.0)) == np.float32(1) / (np.float32(1) + np.float32(1e-6)) < 1


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_entry_points_in_header_and_binding(lib):
    from nerf_simple_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for fn in NEW:
        assert re.search(r"\b%s\s*\(" % fn, header), fn
        assert fn in _lib.EXPORTS and hasattr(raw, fn) and getattr(lib, fn).argtypes is not None, fn
    assert lib.nerf_amd_abi_version() == 5 and "#define NERF_AMD_ABI_VERSION 5" in header      # purely additive
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert _lib._SIGNATURES[NEW[0]] == (i64, [i64])
    assert _lib._SIGNATURES[NEW[1]] == (ctypes.c_int, [vp, i64, vp, vp, vp])
    assert _lib._SIGNATURES[NEW[2]] == (ctypes.c_int, [vp, vp, vp, vp, i64, vp, vp, vp])
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    # the header describes the record, the chain and the attempted-step rule
    for phrase in ("max_norm", "steps skipped", "steps clipped", "fl32(sqrt(S))", "ATTEMPTED step", "1e-6"):
        assert phrase in header, phrase


def test_entry_points_refuse_before_any_launch(lib):
    """Every call here is refused (-1), an empty problem (0) or a size query: every pointer is NULL or a fake address that is
    never dereferenced, so no GPU is needed."""
    EINVAL, null, P, odd = -1, None, ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)
    assert lib.nerf_amd_grad_guard_workspace_bytes(-1) == EINVAL
    sizes = {lib.nerf_amd_grad_guard_workspace_bytes(n) for n in (0, 1, 595844, 2 ** 33)}
    assert len(sizes) == 1 and min(sizes) >= 256 * 8 and min(sizes) % 256 == 0      # one double per workgroup, whatever n is
    assert lib.nerf_amd_grad_guard(P, -1, P, P, null) == EINVAL
    assert lib.nerf_amd_grad_guard(P, 4, P, null, null) == EINVAL                   # no record
    assert lib.nerf_amd_grad_guard(P, 4, P, odd, null) == EINVAL                    # the record is 16-byte aligned
    assert lib.nerf_amd_grad_guard(P, 4, null, P, null) == EINVAL                   # no workspace
    assert lib.nerf_amd_grad_guard(P, 4, ctypes.c_void_p(0x1004), P, null) == EINVAL
    assert lib.nerf_amd_grad_guard(null, 4, P, P, null) == EINVAL                   # gradients missing
    assert lib.nerf_amd_grad_guard(ctypes.c_void_p(0x1002), 4, P, P, null) == EINVAL
    assert lib.nerf_amd_grad_guard(null, 0, null, P, null) == EINVAL                # n == 0 still fills the record
    assert lib.nerf_amd_adam_step_guarded(P, P, P, P, -1, P, P, null) == EINVAL
    assert lib.nerf_amd_adam_step_guarded(P, P, P, P, 4, P, null, null) == EINVAL
    assert lib.nerf_amd_adam_step_guarded(P, P, P, P, 4, P, odd, null) == EINVAL
    assert lib.nerf_amd_adam_step_guarded(null, null, null, null, 0, null, null, null) == EINVAL     # the record comes first
    assert lib.nerf_amd_adam_step_guarded(null, null, null, null, 0, null, P, null) == 0
    for k in range(5):
        args = [P] * 6
        args[k if k < 4 else 5] = null
        assert lib.nerf_amd_adam_step_guarded(*args[:4], 4, args[5], P, null) == EINVAL, k
