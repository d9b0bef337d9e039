"""GPU tests of the e4m3 dW products (csrc/dw_gemm_f8.hip) on exact integers and in poisoned / uninitialised buffers.

tests/test_gpu_storage.py bounds what the 8-bit products add to the storage form's own rounding, on buffers the project's own
producers wrote into zeroed memory.  That leaves unseen: which exponent byte of a group of four a tile reads (the producers
write four equal ones), the split-K edge cases, whatever the kernel reads that nobody wrote (production allocates with
torch.empty), and the pads nobody should read.  Here:

  1. operands that are integers under independently drawn power-of-two exponents, every byte around them poisoned
     (tests/storage_model.py ``crafted``): the 595,844 gradients must EQUAL the float64 products, tolerance zero -- the
     model's docstring says why they can, tests/test_storage_model_cpu.py that these inputs tell a subtly wrong kernel from
     a right one;
  2. the real producers and the consumer in buffers pre-filled with 0xFF, at sizes whose last slab has one block only;
  3. the graphed e4m3 step the same way.

What they found: the exponent byte 0xFF (e8m0's NaN) turns the scaled MFMA's result into NaN even over zero data
(profiles/f8_probe_accumulator.txt), and the kernel read the exponents of BOTH blocks of the last slab where only the first has a
point -- bytes the narrow operands' producer never writes.  The kernel now masks them.
"""
import numpy as np
import pytest
import torch

import storage_model as S
import test_gpu_storage as chain
import train_chain_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


NAMES = [k for k, _ in M.PARAM_SPECS]
STARTS = np.array([M.OFFSETS[k][0] for k in NAMES])


def _must_equal(got, want, tag):
    got = got.astype(np.float64)
    assert got.shape == want.shape == (595844,)
    wrong = np.flatnonzero(~(got == want))                                  # NaN counts as wrong
    if wrong.size:
        where = sorted({NAMES[i] for i in np.searchsorted(STARTS, wrong, side="right") - 1})
        detail = [(int(i), float(got[i]), float(want[i])) for i in wrong[:8]]
        raise AssertionError(f"{tag}: {wrong.size} of 595,844 entries differ ({int(np.isnan(got).sum())} NaN), in {where}; "
                             f"first (index, got, want): {detail}")


@pytest.mark.parametrize("P", S.INT_SIZES)
def test_e4m3_products_on_exact_integers(dev, P):
    """grads must EQUAL the float64 products of integers in [-2, 2] under exponent bytes drawn independently per (layer,
    32-point block, fragment) from {126, 127, 128}: the whole vector, tolerance zero, bucket 0 and buckets 1 then 2 after one
    ..._begin, with the narrow operands (a) as crafted images with exponents of their own, no conversion, and (b) as integer
    bf16 rows and an integer d_raw through nerf_amd_param_gradients_convert_e4m3(which = 3) into a scratch full of 0xFF.
    Around the operands: e4m3 NaN (0x7F) in the data of points >= P and of chunks past an operand's width, 0xFF (e8m0 NaN) in
    the exponent bytes of blocks with no point and of fragments past the width, in the mask region and in every gap, 7 in the
    pad columns inside a loaded chunk, 32 NaN rows behind the bf16 rows, grads pre-filled with NaN.  Sizes: storage_model.INT_SIZES.

    The largest case (P = 36,928) holds 2 x 95 MB on the device and, on the host, their int8 sources and one float64 operand
    pair at a time."""
    from nerf_simple_amd import _lib
    lib = _lib.lib()
    c = S.crafted(P, 2000 + P)
    # every partial sum, in any order, is exact (storage_model's docstring): the analogue of the bf16 test's |want| < 2^24
    assert c["largest_mass"] < S.ACCUMULATOR_EXACT_RATIO * S.MIN_PRODUCT and np.abs(c["want_crafted"]).max() <= c["largest_mass"]
    ints = c["ints"]
    up = lambda a: torch.from_numpy(a).to(dev)
    acts, dys = up(c["acts"]), up(c["dys"])
    assert acts.numel() == lib.nerf_amd_train_activation_bytes_e4m3(P) and dys.numel() == lib.nerf_amd_train_gradient_bytes_e4m3(P)
    n8 = int(lib.nerf_amd_param_gradients_scratch_e4m3_bytes(P))
    assert c["scratch8"].size == n8
    d_raw = up(ints["d_raw"]).contiguous()
    rows = {}
    for W in (64, 32):
        r = np.concatenate([ints[W].astype(np.float32), np.full((32, W), np.nan, dtype=np.float32)])
        rows[W] = up(r).bfloat16().contiguous()
        assert rows[W].shape == (P + 32, W) and bool(torch.isnan(rows[W][P:]).all())
    st, ptr, ck = _lib.stream_ptr(dev), _lib.ptr, _lib.check
    nscratch = max(int(lib.nerf_amd_param_gradients_scratch_bytes(P)), 16)
    for way in ("crafted", "converted"):
        for buckets in ((0,), (1, 2)):
            scratch = torch.full((nscratch,), 0xFF, dtype=torch.uint8, device=dev)
            scratch8 = up(c["scratch8"]) if way == "crafted" else torch.full((n8,), 0xFF, dtype=torch.uint8, device=dev)
            grads = torch.full((M.PARAM_COUNT,), float("nan"), device=dev)
            ck(lib.nerf_amd_param_gradients_begin(ptr(d_raw), ptr(scratch), ptr(grads), P, st), "begin")
            if way == "converted":
                ck(lib.nerf_amd_param_gradients_convert_e4m3(ptr(rows[64]), ptr(rows[32]), ptr(scratch), ptr(scratch8), P, 3, st),
                   "convert")
            for bucket in buckets:
                ck(lib.nerf_amd_param_gradients_finish_e4m3(ptr(acts), ptr(dys), ptr(scratch8), ptr(grads), P, bucket, st), "finish")
            torch.cuda.synchronize()
            _must_equal(grads.cpu().numpy(), c["want_" + way], f"P={P} {way} narrow operands, buckets {buckets}")
            if way == "converted":
                # rows_to_e4m3_kernel: +-1, +-2 and the pad's 7 are exact under the exponent it chooses
                for W, (vals, _, _, _) in S.decode_scratch(scratch8.cpu().numpy(), P).items():
                    want = ints[W].astype(np.float64)
                    if W == 16:
                        want[:, 4:] = 0                       # ..._begin packs d_raw into columns 0..3 of zero rows
                    assert np.array_equal(vals, want), (P, W)
    print(f"E4M3 INTEGERS P={P}: all 595,844 entries exact in 2 x 2 forms; largest |entry| {float(np.abs(c['want_crafted']).max())}")


def _check_layer2(a8, tag):
    """tests/test_gpu_storage.py test_e4m3_products_add_nothing_of_their_own's rule, unchanged: finite, and within 2^-11 of the
    tensor's largest entry of the float64 products of the decoded operands (only what has a point is decoded)."""
    from nerf_simple_amd.utils.nets import Nerf
    want = chain.expected_grads(a8, None)
    off = 0
    for k, p in Nerf().named_parameters():
        n = p.numel()
        got = a8["grads"][off:off + n].reshape(p.shape).astype(np.float64)
        off += n
        w = want[k].reshape(p.shape)
        assert np.isfinite(w).all(), (tag, k)
        assert np.isfinite(got).all(), (tag, k, int((~np.isfinite(got)).sum()), got.size)
        scale = max(np.abs(w).max(), 1e-30)
        assert np.abs(got - w).max() <= 2.0 ** -11 * scale + 1e-12, (tag, k, float(np.abs(got - w).max() / scale))
    assert off == a8["grads"].size


@pytest.mark.parametrize("buckets", [False, True], ids=["bucket0", "buckets12"])
@pytest.mark.parametrize("B,N", [(3, 7), (3, 32), (25, 24), (1, 64)])
def test_e4m3_chain_in_uninitialised_buffers(dev, synthetic, B, N, buckets):
    """The real producers and the consumer with acts, dys, scratch and scratch8 pre-filled with 0xFF (a training step allocates
    them with torch.empty).  P = 21, 96, 600: the last slab's second block has no point, so the narrow operands' producer
    writes no exponent for it; P = 64: it has."""
    a8 = chain.run_chain(dev, synthetic, B, N, True, buckets=buckets, fill=0xFF)
    _check_layer2(a8, (B, N, buckets))


def test_graphed_e4m3_step_in_uninitialised_buffers(dev, synthetic):
    """GraphedTrainStep(storage='e4m3') at B = 3, N = 32 (96 points: three blocks), its pass's acts, dys and scratch8 filled with
    0 or with 0xFF before the first step: the same loss to the last bit, finite gradients, equal up to the order of the float
    atomics (2e-5 of the largest entry: test_e4m3_buckets_are_the_whole's rule)."""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedTrainStep
    from nerf_simple_amd.utils.nets import Nerf
    from nerf_simple_amd.utils.xyz import camera_rays, spherical_to_pose
    B, N = 3, 32
    gen = torch.Generator().manual_seed(3)
    pose = torch.from_numpy(spherical_to_pose(4, -30, 0)).float()
    rays = camera_rays([pose], [2, 2, synthetic.focal_from_fov(2)]).float()[:B].contiguous().to(dev)
    gt, u = torch.rand(B, 3, generator=gen).to(dev), torch.rand(B, N, generator=gen).to(dev)
    res = {}
    for fill in (0, 0xFF):
        net = Nerf(precision="bf16").to(dev)
        net.load_state_dict(synthetic.synthetic_state_dict(0, "default"))
        stepper = GraphedTrainStep(net, FusedAdam(net, lr=5e-4), B, N, storage="e4m3")
        for buf in (stepper.passes[0].acts, stepper.passes[0].dys, stepper.passes[0].scratch8):
            buf.fill_(fill)
        loss = float(stepper.step(rays, gt, u=u))
        torch.cuda.synchronize()
        res[fill] = (loss, stepper.grads.detach().cpu().numpy().astype(np.float64))
    assert res[0][0] == res[0xFF][0] and np.isfinite(res[0][0])
    g0, g1 = res[0][1], res[0xFF][1]
    assert np.isfinite(g0).all() and np.isfinite(g1).all(), (int((~np.isfinite(g0)).sum()), int((~np.isfinite(g1)).sum()))
    scale = np.abs(g0).max()
    assert scale > 0 and np.abs(g0 - g1).max() <= 2e-5 * scale, float(np.abs(g0 - g1).max() / scale)
