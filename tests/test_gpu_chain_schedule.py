"""The chunk schedule of the 16-bit MFMA chain (csrc/mlp16_chain.h chunk_step) only decides WHEN instructions issue.

A wave's issue priority falls as it advances through a weight chunk, so that the two waves of a SIMD stay in step; the
instructions and their operands are what they were.  Nothing a kernel computes may therefore depend on it, and a
schedule that let a wave read a weight buffer before its barrier, or the ring before its samples are in, would show as
a launch that differs from its neighbour, from the two-launch path or from the sigma-only kernel.  Small shapes, every
tile geometry: one point, exactly one tile, one and a half tiles, a ragged ray length, many rays per tile with a partial
last tile.  (tests/test_gpu_parity.py test_fused_render_random_shapes already holds the fused render against the
two-launch path for one ray of one sample in fp16; that pair is not repeated here.)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("rgb", "disp", "alpha", "acc", "w")
SHAPES = [(1, 1), (2, 128), (3, 128), (5, 100), (9, 3)]
SEED, OFFSET = 11, 300
CASES = [(p, B, N) for p in ("fp16", "bf16") for B, N in SHAPES]
# asserted for this shape by tests/test_gpu_parity.py::test_fused_render_random_shapes
FUSED_CASES = [c for c in CASES if c != ("fp16", 1, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scene(dev, synthetic):
    """rays of one small view and one packed network per precision, shared by every case and left unchanged"""
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils.nets import Nerf
    from nerf_simple_amd.utils.xyz import camera_rays, spherical_to_pose
    pose = torch.from_numpy(spherical_to_pose(4, -30, 20)).float()
    rays = camera_rays([pose], [8, 8, synthetic.focal_from_fov(8)]).float().contiguous().to(dev)
    nets = {}
    for precision in ("fp16", "bf16"):
        net = Nerf(precision=precision).to(dev)
        net.load_state_dict(synthetic.synthetic_state_dict(0, "structured"))
        nets[precision] = net
    return rays, nets, _lib


def bits(t):
    return t.contiguous().view(torch.int32)


def outputs(B, N, fill, dev):
    return [torch.full(s, fill, device=dev) for s in ((B, 3), (B,), (B, N), (B,), (B, N))]


def fused(scene, dev, precision, B, N, fill):
    rays, nets, _lib = scene
    code = _lib.precision_code(precision)
    out = outputs(B, N, fill, dev)
    tb = torch.linspace(2, 6, N + 1).to(dev)
    _lib.check(_lib.lib().nerf_amd_render_forward(_lib.ptr(rays[:B].contiguous()), None, _lib.ptr(tb),
                                                  _lib.ptr(nets[precision].packed_weights(code)), code, _lib.FLAG_DEVICE_RNG,
                                                  SEED, OFFSET, *[_lib.ptr(x) for x in out], None, B, N, _lib.stream_ptr(dev)),
               "render_forward")
    return out


def two_launch(scene, dev, precision, B, N, fill):
    rays, nets, _lib = scene
    lib, code, st = _lib.lib(), _lib.precision_code(precision), _lib.stream_ptr(dev)
    r = rays[:B].contiguous()
    tb = torch.linspace(2, 6, N + 1).to(dev)
    raw, ts = torch.empty(B, N, 4, device=dev), torch.empty(B, N, device=dev)
    _lib.check(lib.nerf_amd_mlp_forward_rays(_lib.ptr(r), None, _lib.ptr(tb), _lib.ptr(nets[precision].packed_weights(code)), code,
                                             _lib.FLAG_DEVICE_RNG, SEED, OFFSET, _lib.ptr(raw), _lib.ptr(ts), B, N, st),
               "mlp_forward_rays")
    out = outputs(B, N, fill, dev)
    _lib.check(lib.nerf_amd_volume_render_rays(_lib.ptr(raw), _lib.ptr(ts), _lib.ptr(r), *[_lib.ptr(x) for x in out], B, N, st),
               "volume_render_rays")
    return out, raw, ts


def same_bytes(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("precision,B,N", FUSED_CASES)
def test_fused_render_equals_forward_then_compositor(dev, scene, precision, B, N):
    """rgb / disp / alpha / acc / w of the one-launch render are the bytes of nerf_amd_mlp_forward_rays followed by
    nerf_amd_volume_render_rays on the same device jitter.  (At N == 1 the reference's sample axis is empty: alpha
    and w are not written by either path and keep their fill.)"""
    one = fused(scene, dev, precision, B, N, -7.0)
    two, _, _ = two_launch(scene, dev, precision, B, N, -7.0)
    torch.cuda.synchronize()
    assert torch.isfinite(one[0]).all()
    for n, a, b in zip(NAMES, one, two):
        assert same_bytes(a, b), (precision, B, N, n)


@pytest.mark.parametrize("precision,B,N", CASES)
def test_two_consecutive_launches_write_the_same_bytes(dev, scene, precision, B, N):
    """The same launch twice, into buffers with different fill: every byte equal (elements neither launch writes
    would differ by their fill, except where the contract leaves them unwritten: alpha and w at N == 1)."""
    first = fused(scene, dev, precision, B, N, -7.0)
    second = fused(scene, dev, precision, B, N, 5.0)
    raw1 = two_launch(scene, dev, precision, B, N, -7.0)[1]
    raw2 = two_launch(scene, dev, precision, B, N, 5.0)[1]
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, first, second):
        if N == 1 and n in ("alpha", "w"):
            assert bool((a == -7.0).all()) and bool((b == 5.0).all()), (precision, B, N, n)
            continue
        assert same_bytes(a, b), (precision, B, N, n)
    assert same_bytes(raw1, raw2), (precision, B, N)


@pytest.mark.parametrize("precision,B,N", CASES)
def test_density_sigma_is_column_3_of_the_forward(dev, scene, precision, B, N):
    """The sigma-only kernel (csrc/density.hip, the same chain on a shorter plan) on the B * N sample positions of the
    case: the bytes of column 3 of nerf_amd_mlp_forward's raw output for the same points."""
    rays, nets, _lib = scene
    lib, code, st = _lib.lib(), _lib.precision_code(precision), _lib.stream_ptr(dev)
    _, _, ts = two_launch(scene, dev, precision, B, N, 0.0)
    r = rays[:B]
    pts = (r[:, None, :3] + ts[..., None] * r[:, None, 3:]).reshape(-1, 3)
    pts6 = torch.cat([pts, r[:, None, 3:].expand(B, N, 3).reshape(-1, 3)], 1).contiguous()
    P = B * N
    packed = nets[precision].packed_weights(code)
    raw = torch.empty(P, 4, device=dev)
    _lib.check(lib.nerf_amd_mlp_forward(_lib.ptr(pts6), _lib.ptr(packed), _lib.ptr(raw), P, code, st), "mlp_forward")
    sigma = torch.full((P + 4,), -7.0, device=dev)
    assert lib.nerf_amd_density_forward(_lib.ptr(pts6), 6, _lib.ptr(packed), code, _lib.ptr(sigma), P, st) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(raw).all()
    assert same_bytes(sigma[:P], raw[:, 3]), (precision, B, N)
    assert bool((sigma[P:] == -7.0).all())
