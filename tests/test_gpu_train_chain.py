"""GPU tests that pin the bf16 training kernels (the default storage form: train_step, GraphedTrainStep) stage by stage to
their STORED operands (tests/train_chain_model.py).

  1. staged, kernel-produced buffers: forward -> compositor backward -> dX chain -> dW through the C ABI; every saved
     activation, raw, every stored dY and all 24 gradient tensors, element by element, against the float64 evaluation of the
     stage's own stored inputs with the derived half-ulp / fp32-sum bound.  The worst |got - y| / bound per stage is printed
     (an output, not a tolerance) and must be <= 1 everywhere;
  2. the 14 products and the bias sums on exact integers: host-crafted operands in [-2, 2] (exact in bf16, every partial sum
     an integer below 2^24, so the fp32 result is exact in ANY summation order, float atomics included): all 595,844 entries
     must EQUAL the integer products, at sizes chosen for the split-K slice arithmetic, in all three call forms.

The end-to-end rule for the parameter gradients (FACTOR_16 x the CPU emulation's error) sits with the oracle comparisons in
tests/test_gpu_training.py.
"""
import numpy as np
import pytest
import torch

import storage_model as S
import train_chain_model as M
from test_gpu_storage import run_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- 1. staged -----------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (3, 7), (5, 51), (257, 1), (25, 24), (37, 65), (64, 64)]          # P = 1, 21, 255, 257, 600, 2405, 4096


@pytest.mark.parametrize("zero_enc", [False, True], ids=["full", "enc0"])
@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("B,N", SIZES)
def test_every_stage_against_its_stored_operands(dev, synthetic, B, N, kind, zero_enc):
    """Weight sets: default, structured, and each with the encoder columns of the skip and the colour layer zeroed (layers
    1..9 are then exact in their stored operands; with the full weights the stored encoder rows are the operand and
    delta_enc is added, train_chain_model docstring).  The dW stage stays at P <= 4096 so that delta is far below the
    weight of one 32-point slab; larger sizes belong to the exact-integer test below.

    At N = 1 the reference composites an empty sample axis (csrc/composite_device.h): the compositor's d_raw is identically
    zero and so is everything behind it.  Those sizes run twice: with the compositor's own d_raw (every dY and every
    gradient must then be exactly zero) and with a random upstream gradient of 1e-3 in its place, which is the run the
    non-triviality assertions are made on."""
    sd = synthetic.synthetic_state_dict(5, kind)
    if zero_enc:
        sd = M.zero_encoder_columns(sd)
    if N == 1:
        a = run_chain(dev, synthetic, B, N, False, kind, sd=sd)
        assert not a["d_raw"].any() and not a["grads"].any()
        assert not any(y.any() for y in M.decode_bf16_layers(a["dys"], B))
        _check_stages(a, sd, f"{kind} {'enc0' if zero_enc else 'full'} (compositor's zero d_raw)", zero_enc, nontrivial=False)
    g = torch.randn(B * N, 4, generator=torch.Generator().manual_seed(5)) * 1e-3 if N == 1 else None
    a = run_chain(dev, synthetic, B, N, False, kind, sd=sd, d_raw_in=g)
    _check_stages(a, sd, f"{kind} {'enc0' if zero_enc else 'full'}", zero_enc, nontrivial=B * N >= 255)


def _check_stages(a, sd, tag, zero_enc, nontrivial):
    P = a["P"]
    assert a["acts"].size == M.acts_bf16_bytes(P) + 10 * M.act_tiles(P) * 8192
    bufs = dict(X=M.decode_bf16_layers(a["acts"], P), masks=M.decode_masks(a["acts"], P), raw=a["raw"].reshape(P, 4),
                dY=M.decode_bf16_layers(a["dys"], P), dsr=M.decode_d_raw_rows(a["scratch"], P), d_raw=a["d_raw"],
                posx=a["posx"], posd=a["posd"], grads=a["grads"])
    if zero_enc:
        W = M.w16(sd)
        for L in (5, 9):
            assert not np.any(M.forward_stage(L, W, [x.astype(np.float64) for x in bufs["X"]],
                                              bufs["posx"][:, :63].astype(np.float64), bufs["posd"][:, :27].astype(np.float64))[3])
    res = M.check_chain(bufs, sd)
    print(M.report(res, f"STAGES P={P} {tag}:"))
    for k, v in res.items():
        print(f"    STAGE {k:32s} {v:.4f}")
    assert len(res) == 10 + 9 + 2 + 1 + 10 + 24
    if nontrivial:                                   # 20-80 % of each mask set, no all-zero dY layer
        for L in (0, 1, 2, 3, 4, 5, 6, 7, 9):
            frac = bufs["masks"][L][:, :M.act_width(L)].mean()
            assert 0.2 <= frac <= 0.8, (L, frac)
        for L in range(10):
            assert np.abs(bufs["dY"][L][:, :M.act_width(L)]).max() > 0, L
    bad = {k: v for k, v in res.items() if not v <= 1}
    assert not bad, bad


# ---- 2. dW on exact integers ---------------------------------------------------------------------------------------------
BF16_OF_INT = np.array([0x0000, 0x3F80, 0x4000, 0xC000, 0xBF80], dtype=np.uint16)       # index v (mod 5) for v in -2 .. 2
INT_SIZES = [1, 31, 32, 33,                                        # fewer slabs than workgroups per product
             479, 481, 543, 544, 545, 576, 577, 609, 641,          # 15 .. 20 slabs: around the per-product workgroup shares
             255, 256, 257,                                        # tile edges
             2405, 4096, 36928,
             131072 + 37]                                          # one large ragged case
# ... and every size of the model at which a product has one slab fewer than, as many as, one more than its workgroups on 256
# CUs (smallest and largest share of each of the three launches; the launcher's plan is the model's:
# tests/test_dw_products_cpu.py)
INT_SIZES += [P for P in S.share_edge_sizes(256, **S.BF16_FORM) if P not in INT_SIZES]


def _crafted(P, seed):
    """Integer operands in [-2, 2] and the buffers that hold them, as uint8 / float arrays on the host."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nt = M.act_tiles(P)
    ints = {}
    bufs = {}
    for name in ("X", "dY"):
        v = rng.integers(-2, 3, size=(10, P, 256), dtype=np.int8)
        # features 128..255 of layer 9 (128 wide) are no operand of any product: a finite poison value
        v[9, :, 128:] = 7
        ints[name] = v
        bits = np.full((10, nt * 256, 256), 0xFFFF, dtype=np.uint16)          # granules of points >= P: bf16 NaN
        bits[:, :P] = BF16_OF_INT[v % 5]
        bits[9, :P, 128:] = 0x40E0                                              # 7.0
        blocked = np.ascontiguousarray(bits.reshape(10, nt, 256, 32, 8).transpose(0, 1, 3, 2, 4)).reshape(-1).view(np.uint8)
        bufs[name] = blocked
    for name, w, true in (("posx", 64, 63), ("posd", 32, 27)):
        v = rng.integers(-2, 3, size=(P, w), dtype=np.int8).astype(np.float32)
        v[:, true:] = 7.0                                                       # pad columns: finite, must not be stored
        ints[name] = v
        bufs[name] = np.concatenate([v, np.full((32, w), np.nan, dtype=np.float32)])     # 32 rows of NaN behind row P - 1
    ints["d_raw"] = rng.integers(-2, 3, size=(P, 4), dtype=np.int8).astype(np.float32)
    return ints, bufs


class _AsFloat64:
    """The ten layers of an int8 operand, converted one at a time."""

    def __init__(self, v):
        self.v = v

    def __getitem__(self, L):
        return self.v[L].astype(np.float64)


def test_crafted_buffers_use_the_model_encoder():
    """The fast integer encoder above writes what train_chain_model.encode_bf16_layers writes."""
    ints, bufs = _crafted(300, 1)
    layers = [ints["X"][L].astype(np.float32) for L in range(10)]
    assert np.array_equal(bufs["X"], M.encode_bf16_layers(layers, 300))
    assert np.array_equal(M.decode_bf16_layers(bufs["dY"], 300)[3], ints["dY"][3].astype(np.float32))


@pytest.mark.parametrize("P", INT_SIZES)
def test_param_gradients_on_exact_integers(dev, P):
    """grads must EQUAL the integer products: tolerance zero, the whole 595,844-entry vector, in three call forms -- bucket 0;
    buckets 1 then 2 after one ..._begin; the one-call nerf_amd_param_gradients.  Around the operands: NaN granules for
    points >= P in the last tile, 32 NaN rows behind posx / posd, pad columns (posx 63, posd 27..31, layer 9's features
    128..255) at the finite value 7, the scratch and grads pre-filled with NaN.

    Memory of the largest case (P = 131,109; about 5 KB per point per buffer): acts and dys 2 x 672 MB on the device (plus
    25 MB of encoder rows and scratch), and on the host the same two buffers, their int8 sources (2 x 336 MB) and one
    float64 operand pair at a time (2 x 268 MB).  It is the only case of that size."""
    from nerf_simple_amd import _lib
    lib = _lib.lib()
    ints, bufs = _crafted(P, 1000 + P)
    f8 = lambda a: np.asarray(a, dtype=np.float64)
    dsr = np.zeros((P, 4))
    dsr[:] = ints["d_raw"]
    want, _ = M.expected_param_grads(_AsFloat64(ints["X"]), _AsFloat64(ints["dY"]), f8(ints["posx"]), f8(ints["posd"]),
                                     dsr, f8(ints["d_raw"]), with_mass=False)
    assert np.array_equal(want, np.round(want)) and np.abs(want).max() < 2 ** 24
    nbytes = int(lib.nerf_amd_train_activation_bytes(P))
    assert nbytes == bufs["X"].size + 10 * M.act_tiles(P) * 8192

    def dev_buf(b):
        t = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)        # the mask region: not read by the products
        t[:b.size] = torch.from_numpy(b).to(dev)
        return t

    acts, dys = dev_buf(bufs["X"]), dev_buf(bufs["dY"])
    posx = torch.from_numpy(bufs["posx"]).to(dev).bfloat16().contiguous()
    posd = torch.from_numpy(bufs["posd"]).to(dev).bfloat16().contiguous()
    assert posx.shape == (P + 32, 64) and posd.shape == (P + 32, 32) and bool(torch.isnan(posx[P:]).all())
    d_raw = torch.from_numpy(ints["d_raw"]).to(dev).contiguous()
    st, ptr, ck = _lib.stream_ptr(dev), _lib.ptr, _lib.check
    nscratch = max(int(lib.nerf_amd_param_gradients_scratch_bytes(P)), 16)
    names = [k for k, _ in M.PARAM_SPECS]
    starts = np.array([M.OFFSETS[k][0] for k in names])
    for form in ("bucket 0", "buckets 1, 2", "one call"):
        scratch = torch.full((nscratch,), 0xFF, dtype=torch.uint8, device=dev)
        grads = torch.full((M.PARAM_COUNT,), float("nan"), device=dev)
        if form == "one call":
            ck(lib.nerf_amd_param_gradients(ptr(d_raw), ptr(acts), ptr(dys), ptr(posx), ptr(posd), ptr(scratch), ptr(grads), P, st),
               "param_gradients")
        else:
            ck(lib.nerf_amd_param_gradients_begin(ptr(d_raw), ptr(scratch), ptr(grads), P, st), "begin")
            for bucket in ((0,) if form == "bucket 0" else (1, 2)):
                ck(lib.nerf_amd_param_gradients_finish_bucket(ptr(acts), ptr(dys), ptr(posx), ptr(posd), ptr(scratch), ptr(grads),
                                                              P, bucket, st), "finish_bucket")
        torch.cuda.synchronize()
        got = grads.cpu().numpy().astype(np.float64)
        assert got.shape == want.shape == (595844,)
        wrong = np.flatnonzero(~(got == want))                                  # NaN counts as wrong
        if wrong.size:
            where = sorted({names[i] for i in np.searchsorted(starts, wrong, side="right") - 1})
            detail = [(int(i), float(got[i]), float(want[i])) for i in wrong[:8]]
            raise AssertionError(f"P={P} {form}: {wrong.size} of 595,844 entries differ, in {where}; first (index, got, want): {detail}")
        packed = M.decode_d_raw_rows(scratch.cpu().numpy(), P)
        assert np.array_equal(packed[:, :4], ints["d_raw"]) and not packed[:, 4:].any(), (P, form)
    print(f"INTEGERS P={P}: all 595,844 entries exact in three forms; largest |entry| {int(np.abs(want).max())}")
