"""Gradients with respect to the inputs, the parts that need no GPU: the C ABI's argument checks, the bf16 emulation
model's bound, and the float64 yardstick itself against central finite differences."""
import ctypes

import pytest
import torch

import input_grad_model as M


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    return _lib.lib()


def _p(n=1):
    return ctypes.c_void_p(16 * n)        # a non-null address no call below may dereference: every one fails its checks first


def test_input_gradient_entries_are_exported(lib):
    for name in ("nerf_amd_input_gradients", "nerf_amd_query_points_backward", "nerf_amd_gamma_backward",
                 "nerf_amd_positional_encoder_backward"):
        assert hasattr(lib, name)
    assert lib.nerf_amd_abi_version() == 5          # purely additive


def test_input_gradients_argument_errors(lib):
    EINVAL = -1
    # negative sizes, missing pointers, mixed modes
    assert lib.nerf_amd_input_gradients(_p(), _p(), _p(), None, None, _p(), None, -1, 1, None) == EINVAL
    assert lib.nerf_amd_input_gradients(None, _p(), _p(), None, None, _p(), None, 4, 1, None) == EINVAL
    assert lib.nerf_amd_input_gradients(_p(), None, _p(), None, None, _p(), None, 4, 1, None) == EINVAL
    assert lib.nerf_amd_input_gradients(_p(), _p(), _p(), None, None, None, None, 4, 1, None) == EINVAL
    assert lib.nerf_amd_input_gradients(_p(), _p(), _p(), _p(), None, _p(), None, 4, 1, None) == EINVAL    # pts and rays
    assert lib.nerf_amd_input_gradients(_p(), _p(), None, _p(), None, _p(), _p(), 4, 2, None) == EINVAL    # rays without ts
    assert lib.nerf_amd_input_gradients(_p(), _p(), None, _p(), _p(), _p(), None, 4, 2, None) == EINVAL    # no d_rays
    assert lib.nerf_amd_input_gradients(_p(), _p(), None, _p(), _p(), _p(), _p(), 4, 0, None) == EINVAL    # N <= 0
    assert lib.nerf_amd_input_gradients(_p(), _p(), None, _p(), _p(), _p(), _p(), 5, 2, None) == EINVAL    # P % N
    # empty input: nothing to do, nothing launched
    assert lib.nerf_amd_input_gradients(None, None, _p(), None, None, None, None, 0, 1, None) == 0
    assert lib.nerf_amd_input_gradients(None, None, None, None, None, None, None, 0, 4, None) == 0

    assert lib.nerf_amd_query_points_backward(_p(), _p(), _p(), _p(), -1, 4, None) == EINVAL
    assert lib.nerf_amd_query_points_backward(_p(), _p(), _p(), _p(), 3, 0, None) == EINVAL
    assert lib.nerf_amd_query_points_backward(_p(), None, _p(), _p(), 3, 4, None) == EINVAL
    assert lib.nerf_amd_query_points_backward(_p(), _p(), _p(), None, 3, 4, None) == EINVAL
    assert lib.nerf_amd_query_points_backward(None, None, None, None, 0, 4, None) == 0

    assert lib.nerf_amd_gamma_backward(_p(), 1, _p(), _p(), -1, 4, None) == EINVAL
    assert lib.nerf_amd_gamma_backward(_p(), -1, _p(), _p(), 3, 4, None) == EINVAL
    assert lib.nerf_amd_gamma_backward(_p(), 1, _p(), _p(), 3, -1, None) == EINVAL
    assert lib.nerf_amd_gamma_backward(_p(), 1, None, _p(), 3, 4, None) == EINVAL
    assert lib.nerf_amd_gamma_backward(None, 1, None, None, 0, 4, None) == 0

    assert lib.nerf_amd_positional_encoder_backward(_p(), _p(), _p(), _p(), -1, 10, 4, None) == EINVAL
    assert lib.nerf_amd_positional_encoder_backward(_p(), _p(), _p(), _p(), 3, -1, 4, None) == EINVAL
    assert lib.nerf_amd_positional_encoder_backward(_p(), _p(), None, _p(), 3, 10, 4, None) == EINVAL
    assert lib.nerf_amd_positional_encoder_backward(None, None, None, None, 0, 10, 4, None) == 0


def _small_case(seed=0, B=6, N=16):
    from nerf_simple_amd.utils import synthetic
    from nerf_simple_amd.utils.xyz import camera_rays, spherical_to_pose
    sd = synthetic.synthetic_state_dict(0, "structured")
    pose = torch.from_numpy(spherical_to_pose(4, -30, 0)).float()
    rays = camera_rays([pose], [8, 8, synthetic.focal_from_fov(8)])[::64 // B][:B]
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(B, N, generator=g)
    target = torch.rand(B, 3, generator=g)
    return sd, rays, u, target


def test_emulation_bound_is_finite_and_nonzero():
    sd, rays, u, target = _small_case()
    N = u.shape[1]
    g64 = M.rays_grad(M.exact_forward, sd, rays, N, target, torch.float64, u=u)
    g32 = M.rays_grad(M.exact_forward, sd, rays, N, target, torch.float32, u=u)
    g16 = M.rays_grad(M.emulated_forward, sd, rays, N, target, torch.float32, u=u)
    b32, b16 = M.bound_fp32(g32, g64), M.bound_bf16(g16, g32, g64)
    assert 0 < b32 < 1e-2, b32
    assert b32 < b16 < 1.0, (b32, b16)                    # bf16 operands cost more than fp32 round-off, and stay useful
    assert float(g64.abs().max()) > 0


def test_float64_ray_gradients_match_finite_differences():
    """The yardstick: float64 autograd of the oracle's render (utils/rendering.py:13-45) against central differences."""
    sd, rays, u, target = _small_case(B=4, N=16)
    sd64 = M.cast_sd(sd, torch.float64)
    N = u.shape[1]
    r64 = rays.double()
    g = M.rays_grad(M.exact_forward, sd, rays, N, target, torch.float64, u=u)

    def loss(r):
        with torch.no_grad():
            return float(M.ray_loss(M.render(M.exact_forward, sd64, r, N, u=u), target))

    h = 1e-8       # small: a step of 1e-6 moves a sample by ~6e-6, sin(2^9 x) by 3e-3, and crosses ReLU kinks
    fd = torch.zeros_like(r64)
    for i in range(r64.shape[0]):
        for j in range(6):
            e = torch.zeros_like(r64)
            e[i, j] = h
            fd[i, j] = (loss(r64 + e) - loss(r64 - e)) / (2 * h)
    assert M.rel_err(fd, g) < 1e-6, (fd, g)
