"""CPU tests of tests/train_chain_model.py: the layout transcriptions, and the evidence that the stage-by-stage rule the
GPU tests apply (tests/test_gpu_train_chain.py) passes correct arithmetic in more than one summation order and FAILS, in the
stage where it was planted, on each of the defects such kernels are prone to."""
import functools

import numpy as np
import pytest
import torch

import input_grad_model as IG
import train_chain_model as M


def _act_elem_offset(L, p, f, P):
    """csrc/nerf_layout.h act_elem_offset, transcribed term by term."""
    tiles = (P + 255) // 256
    layer_stride = tiles * 256 * 512
    return L * layer_stride + (p // 256) * (256 * 512) + ((f // 8) * 256 + p % 256) * 16 + (f % 8) * 2


@pytest.mark.parametrize("P", [1, 255, 256, 257, 600])
def test_layout_round_trip_and_offsets(P):
    rng = np.random.Generator(np.random.PCG64(P))
    layers = [M.round_bf16(rng.standard_normal((P, 256)).astype(np.float32)) for _ in range(10)]
    buf = M.encode_bf16_layers(layers, P)
    assert buf.dtype == np.uint8 and buf.size == M.acts_bf16_bytes(P) == 10 * ((P + 255) // 256) * 131072
    back = M.decode_bf16_layers(buf, P)
    for L in range(10):
        assert np.array_equal(back[L].view(np.uint32), layers[L].view(np.uint32)), L
    u16 = buf.view(np.uint16)
    for _ in range(2000):
        L, p, f = int(rng.integers(10)), int(rng.integers(P)), int(rng.integers(256))
        off = _act_elem_offset(L, p, f, P)
        assert off % 2 == 0 and u16[off // 2] == M.f32_to_bf16_bits(layers[L][p:p + 1, f])[0], (L, p, f)
    # granules of points >= P in the last tile hold the filler, and nothing else does
    nt = (P + 255) // 256
    pad = buf.view(np.uint16).reshape(10, nt, 32, 256, 8)[:, -1, :, P - (nt - 1) * 256:, :]
    assert (pad == 0xFFFF).all()
    assert np.count_nonzero(u16 == 0xFFFF) == pad.size


def test_mask_decode_is_the_documented_layout():
    """decode_masks against the bit-by-bit loop of the layout comment (nerf_layout.h), on random dwords, ragged P."""
    P = 600
    nt = 3
    rng = np.random.Generator(np.random.PCG64(1))
    words = rng.integers(0, 2 ** 32, size=(10, nt, 4, 512), dtype=np.uint64).astype(np.uint32)
    host = np.concatenate([np.zeros(M.acts_bf16_bytes(P), dtype=np.uint8), words.reshape(-1).view(np.uint8)])
    got = M.decode_masks(host, P)
    tid = np.arange(512)
    wave, lane = tid >> 6, tid & 63
    for L in (0, 5, 9):
        for tile in range(nt):
            for cb in range(2):
                pt = tile * 256 + wave * 32 + cb * 16 + (lane & 15)
                ok = pt < P
                for Q in range(8):
                    for j in range(4):
                        for e in range(2):
                            feat = 32 * Q + 16 * (j >> 1) + 4 * (lane >> 4) + 2 * (j & 1) + e
                            bit = (words[L, tile, cb * 2 + (Q >> 2)] >> ((Q & 3) * 4 + j + 16 * e)) & 1
                            assert np.array_equal(got[L][pt[ok], feat[ok]], bit[ok].astype(bool)), (L, tile, cb, Q, j, e)


def test_packed_d_raw_rows_decode():
    d = M.round_bf16(np.random.Generator(np.random.PCG64(2)).standard_normal((77, 32)).astype(np.float32))
    scratch = np.concatenate([M.f32_to_bf16_bits(d).reshape(-1).view(np.uint8), np.full(100, 0xAB, dtype=np.uint8)])
    assert np.array_equal(M.decode_d_raw_rows(scratch, 77), d)


def test_ulp_and_rule_edges():
    assert M.ulp_bf16(np.array([1.0, 1.99, 2.0, 0.75]))[0] == 2.0 ** -7
    assert np.array_equal(M.ulp_bf16(np.array([1.0, 1.99, 2.0, 0.75])), 2.0 ** np.array([-7.0, -7, -6, -8]))
    one = np.ones((1, 1))
    # half a bf16 step passes, a whole one does not; a negative stored ReLU output and a nonzero dY under a 0 mask bit are inf
    assert M.stage_ratio(one * (1 + 2.0 ** -8), one, one, 0, True) <= 1
    assert M.stage_ratio(one * (1 + 2.0 ** -7), one, one, 0, True) > 1.9
    assert M.stage_ratio(-one * 2.0 ** -20, one * 2.0 ** -20, one, 0, True, relu=True) == float("inf")
    assert M.stage_ratio(one * 2.0 ** -20, -one, one, 0, True, relu=True) == float("inf")
    assert M.stage_ratio(one * 2.0 ** -30, one * 2.0 ** -30, one, 0, True, mask=np.zeros((1, 1), dtype=bool)) == float("inf")


def _inputs(synthetic, oracle, kind, P=600, zero_enc=False, pad=7.0):
    sd = synthetic.synthetic_state_dict(5, kind)
    if zero_enc:
        sd = M.zero_encoder_columns(sd)
    v = synthetic.points_in_scene(P, seed=3)
    x, d = oracle.positional_encoder(v, 10, 4)
    posx64 = torch.cat([x.bfloat16().float(), torch.full((P, 1), pad)], dim=1)
    posd32 = torch.cat([d.bfloat16().float(), torch.full((P, 5), pad)], dim=1)
    d_raw = torch.randn(P, 4, generator=torch.Generator().manual_seed(7)) * 1e-3
    return sd, v, posx64, posd32, d_raw


@pytest.mark.parametrize("zero_enc", [False, True])
@pytest.mark.parametrize("order", ["plain", "split"])
@pytest.mark.parametrize("kind", ["default", "structured"])
def test_correct_arithmetic_passes_every_stage(synthetic, oracle, kind, order, zero_enc):
    sd, _, posx64, posd32, d_raw = _inputs(synthetic, oracle, kind, zero_enc=zero_enc)
    bufs = M.emulate_chain(sd, posx64, posd32, d_raw, order=order, seed=11)
    res = M.check_chain(bufs, sd, enc_slack=False)          # the emulation's forward reads the stored rows themselves
    print(M.report(res, f"{kind} {order} zero_enc={zero_enc}:"))
    assert len(res) == 10 + 9 + 2 + 1 + 10 + 24
    bad = {k: v for k, v in res.items() if not v <= 1}
    assert not bad, bad
    for L in range(8):                                       # the case is not trivial
        assert 0.2 <= bufs["masks"][L].mean() <= 0.8, (L, bufs["masks"][L].mean())
        assert np.abs(bufs["dY"][L]).max() > 0


FAULTS = {
    "truncate": {"X[2]"},                                     # truncation instead of round-to-nearest-even in one stored layer
    "swap_k": {"X[3]"},                                       # two swapped k columns
    "flip_mask": {"dY[4]"},                                   # one ReLU mask bit read wrong
    "no_sigma": {"dY[7]"},                                    # the sigma k-step left out
    "drop_slab": {"dW layers_0.4.weight"},                    # one 32-point slab dropped from a product
    "double_slab": {"dW layers_0.6.weight"},                  # ... counted twice
    "bias_tail": {"db layers_1.0.bias"},                      # the last P % 32 points left out of a bias sum
    "skip_col": {"dW skip_conn_layer.0.weight"},              # the skip layer's x part written at column 255
    "posx_leak": {"dW layers_0.0.weight", "db layers_0.0.bias"},   # posx column 63 stored: it lands on the next row's column 0
}


@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_is_caught_in_its_stage(synthetic, oracle, kind, fault):
    sd, _, posx64, posd32, d_raw = _inputs(synthetic, oracle, kind)
    bufs = M.emulate_chain(sd, posx64, posd32, d_raw, order="split", seed=11, fault=fault)
    res = M.check_chain(bufs, sd, enc_slack=False)
    caught = {k for k, v in res.items() if not v <= 1}
    print(fault, {k: res[k] for k in caught})
    assert caught == FAULTS[fault], (fault, {k: res[k] for k in caught})


def test_encoder_slack_is_zero_without_encoder_columns(synthetic, oracle):
    sd, _, posx64, posd32, _ = _inputs(synthetic, oracle, "default", P=40, zero_enc=True)
    W = M.w16(sd)
    X = [np.zeros((40, 256))] * 10
    for L in (5, 9):
        assert not np.any(M.forward_stage(L, W, X, posx64.double().numpy()[:, :63], posd32.double().numpy()[:, :27])[3])
    full = M.w16(synthetic.synthetic_state_dict(5, "default"))
    de = M.forward_stage(5, full, X, posx64.double().numpy()[:, :63], posd32.double().numpy()[:, :27])[3]
    assert de.shape == (40, 256) and (de > 0).all()


def test_chain_emulation_and_autograd_emulation_agree(synthetic, oracle):
    """The explicit emulation of the chain and the autograd emulation that the end-to-end tests use as their error model
    (input_grad_model.emulated_forward(train_heads=True)) are two fp32 evaluations of the same roundings: per tensor they
    differ by far less (a tenth) than either differs from the float64 gradient."""
    sd, v, posx64, posd32, d_raw = _inputs(synthetic, oracle, "default", P=300)
    bufs = M.emulate_chain(sd, posx64, posd32, d_raw, order="plain")
    fwd = functools.partial(IG.emulated_forward, train_heads=True)
    _, g16 = IG.points_grad(fwd, sd, v, d_raw, torch.float32)
    _, g64 = IG.points_grad(IG.exact_forward, sd, v, d_raw, torch.float64)
    _, g16_plain = IG.points_grad(IG.emulated_forward, sd, v, d_raw, torch.float32)
    for name, (off, shape) in M.OFFSETS.items():
        mine = torch.from_numpy(bufs["grads"][off:off + int(np.prod(shape))].reshape(shape))
        e16 = IG.rel_err(g16[name], g64[name])
        assert IG.rel_err(mine, g16[name]) <= 0.1 * e16, (name, IG.rel_err(mine, g16[name]), e16)
    # the keyword changes the head weights' gradients (bf16 d_raw) and leaves the head biases alone (fp32 d_raw)
    assert not torch.equal(g16["sigma_fc.0.weight"], g16_plain["sigma_fc.0.weight"])
    assert torch.equal(g16["sigma_fc.0.bias"], g16_plain["sigma_fc.0.bias"])
    assert torch.equal(g16["color_fc.2.bias"], g16_plain["color_fc.2.bias"])
