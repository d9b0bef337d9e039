"""CPU tests of tests/storage_model.py: the host model of the 8-bit storage form encodes what it decodes, sizes its images as
the library does, poisons only where no operand lives, restates the launcher's share arithmetic -- and its crafted inputs CAN
tell a subtly wrong dW kernel from a right one (selectivity), at every size tests/test_gpu_storage_integers.py runs."""
import numpy as np
import pytest

import storage_model as S
import train_chain_model as M


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    return _lib.lib()                                   # the size functions need no GPU


@pytest.fixture(scope="module", params=S.INT_SIZES)
def crafted(request):
    """One size's crafted inputs, shared by the tests below (the seed of the GPU test)."""
    return S.crafted(request.param, 2000 + request.param)


def test_r_is_the_measured_one():
    """R = 2^24 is what profiles/f8_probe_accumulator.txt records: D - C = 1 for C = 2^k, k = 8..23, and the tie at k = 24."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "f8_probe_accumulator.txt")
    rows = {}
    with open(path) as f:
        for line in f:
            m = re.match(r"\s+k = +(\d+): D - C = (\S+) \(D\[31\]\[31\]: (\S+)\) \| (\S+) \(D\[31\]\[31\]: (\S+)\)", line)
            if m:
                rows[int(m.group(1))] = [float(m.group(i)) for i in range(2, 6)]
    assert sorted(rows) == list(range(8, 25))
    exact = [k for k in sorted(rows) if rows[k] == [1.0, 1.0, 64.0, 64.0]]
    assert exact == list(range(8, 24)) and rows[24][:2] == [0.0, 0.0]
    assert S.ACCUMULATOR_EXACT_RATIO == 2.0 ** (exact[-1] + 1)


def test_int_codes():
    assert np.array_equal(S.E4M3[S.INT_TO_E4M3], np.arange(-16, 17)) and S.INT_TO_E4M3[16] == 0
    assert np.isnan(S.E4M3[S.DATA_POISON]) and S.EXP_POISON == 0xFF


def test_shares_restate_the_launcher():
    """256 workgroups in every launch with slabs to spare; one workgroup per slab where there are fewer slabs than a share; the
    sizes of the GPU test sit at share - 1, share, share + 1 slabs of the smallest and the largest share of each launch."""
    for bucket, n in ((0, 14), (1, 9), (2, 5)):
        w = S.workgroup_shares(1 << 20, bucket)
        assert len(w) == n and sum(w) == 256 and min(w) >= 1
        for edge in (min(w), max(w)):
            for slabs in (edge - 1, edge, edge + 1):
                assert {64 * slabs - 1, 64 * slabs, 64 * slabs + 1} <= set(S.INT_SIZES)
            assert S.workgroup_shares(64 * edge, bucket).count(edge) >= 1
            assert max(S.workgroup_shares(64 * (edge - 1), bucket)) <= edge - 1
    assert S.workgroup_shares(1, 0) == [1] * 14 and S.workgroup_shares(65, 2) == [2] * 5
    assert S.workgroup_shares((1 << 22) * 20, 0)[12] == 21           # the ``need`` clamp: 20 GiB per operand -> 21 slices
    assert {1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 255, 256, 257, 2405, 36928} <= set(S.INT_SIZES)


def test_sizes_are_the_librarys(lib, crafted):
    P = crafted["P"]
    assert crafted["acts"].size == lib.nerf_amd_train_activation_bytes_e4m3(P) == S.f8_acts_total_bytes(P)
    assert crafted["dys"].size == lib.nerf_amd_train_gradient_bytes_e4m3(P) == S.f8_data_bytes(P)
    assert crafted["scratch8"].size == lib.nerf_amd_param_gradients_scratch_e4m3_bytes(P) == S.narrow_offsets(P)[1]


def test_decode_inverts_encode(crafted):
    P, ints, exps = crafted["P"], crafted["ints"], crafted["exps"]
    nb = S.blocks(P)
    for name, image in (("X", crafted["acts"]), ("dY", crafted["dys"])):
        vals, raws, ex = S.decode_e4m3_layers(image, P)
        want = S.Scaled(ints[name], exps[name], P)
        for L in range(10):
            w = M.act_width(L)
            assert np.array_equal(vals[L][:, :w], want[L][:, :w]), (name, L)
            assert np.array_equal(ex[L][:nb, :w // 32], exps[name][L][:, :w // 32]), (name, L)
    for W, (vals, raws, ex, per) in S.decode_scratch(crafted["scratch8"], P).items():
        assert np.array_equal(vals, ints[W] * per) and np.array_equal(S.E4M3[raws], ints[W]), W
        assert np.array_equal(ex[:nb, :(W + 31) // 32], exps[W]), W


def test_poison_sits_only_where_no_operand_lives(crafted):
    """Every byte of the three images is either an operand's (a finite e4m3 code of a point < P and a feature inside the width;
    an exponent byte 126..128 of a block with a point and a fragment inside the width) or poison -- and never both."""
    P = crafted["P"]
    nt, nb = S.tiles(P), S.blocks(P)
    for image in (crafted["acts"], crafted["dys"]):
        data = image[:10 * nt * 65536].reshape(10, nt, 16, 256, 16).transpose(0, 1, 3, 2, 4).reshape(10, nt * 256, 256)
        ex = image[10 * nt * 65536:S.f8_data_bytes(P)].reshape(10, nt * 8, 8)
        for L in range(10):
            w = M.act_width(L)
            assert not np.isnan(S.E4M3[data[L, :P, :w]]).any() and (np.abs(S.E4M3[data[L, :P, :w]]) <= 2).all()
            assert (data[L, P:] == S.DATA_POISON).all() and (data[L, :, w:] == S.DATA_POISON).all()
            assert np.isin(ex[L, :nb, :w // 32], S.EXP_BYTES).all()
            assert (ex[L, nb:] == S.EXP_POISON).all() and (ex[L, :, w // 32:] == S.EXP_POISON).all()
        assert (image[S.f8_data_bytes(P):] == S.MASK_POISON).all()                 # acts: the gap and the mask region
    offs, total = S.narrow_offsets(P)
    seen = np.zeros(total, dtype=bool)
    for W, true in S.NARROW:
        buf = crafted["scratch8"][offs[W]:offs[W] + S.narrow_bytes(W, P)]
        seen[offs[W]:offs[W] + buf.size] = True
        vals, raws, ex, _ = S.decode_e4m3_narrow(buf, W, P)
        nq = (W + 31) // 32
        assert (np.abs(S.E4M3[raws[:, :true]]) <= 2).all() and (S.E4M3[raws[:, true:]] == S.PAD_VALUE).all()
        data = buf[:nt * (W // 16) * 4096].reshape(nt, W // 16, 256, 16).transpose(0, 2, 1, 3).reshape(nt * 256, W)
        assert (data[P:] == S.DATA_POISON).all()
        assert np.isin(ex[:nb, :nq], S.EXP_BYTES).all() and (ex[nb:] == S.EXP_POISON).all() and (ex[:, nq:] == S.EXP_POISON).all()
    assert (crafted["scratch8"][~seen] == S.EXP_POISON).all()


def test_expected_gradients_are_exact_by_construction(crafted):
    """Every entry is a multiple of MIN_PRODUCT below R of them (storage_model's docstring), dense operands at every size; the
    converted form differs from the crafted one in the entries the narrow operands enter and nowhere else."""
    P = crafted["P"]
    assert crafted["density"] == 1.0 and P * S.MAX_PRODUCT < S.ACCUMULATOR_EXACT_RATIO * S.MIN_PRODUCT
    for k in ("want_crafted", "want_converted"):
        w = crafted[k]
        assert w.shape == (M.PARAM_COUNT,) and np.array_equal(w, np.round(w * 4) / 4) and np.abs(w).max() < 2.0 ** 22
        assert np.array_equal(w.astype(np.float32).astype(np.float64), w)
    differ = crafted["want_crafted"] != crafted["want_converted"]
    narrow = np.zeros(M.PARAM_COUNT, dtype=bool)
    for name, cols in (("layers_0.0.weight", slice(0, 63)), ("skip_conn_layer.0.weight", slice(256, 319)),
                       ("color_fc.0.weight", slice(256, 283)), ("sigma_fc.0.weight", slice(0, 256)), ("color_fc.2.weight", slice(0, 128))):
        off, shape = M.OFFSETS[name]
        narrow[off:off + int(np.prod(shape))].reshape(shape)[:, cols] = True
    assert not differ[~narrow].any() and differ.any()


@pytest.mark.parametrize("variant", S.VARIANTS)
def test_selectivity(crafted, variant):
    """A kernel that reads exponent byte Q ^ 1, that swaps the exponents of a slab's two blocks, or that loses a slab changes at
    least one entry of EVERY product that reads the misread operand: the crafted inputs can tell it from a right one.

    Exempt, for lack of anything to misread (and there the wrong byte is a poisoned one, 0xFF, which gives NaN): swap_q on the
    32- and 16-wide operands (one fragment: no byte Q ^ 1 inside the width); swap_blocks at P <= 32 (one block), and for the
    last block of an odd count."""
    P = crafted["P"]
    changes = S.variant_changes(crafted, variant, max_features=64 if P > 512 else None)
    if variant.startswith("drop"):
        assert len(changes) == len(S.PRODUCTS) == 24
    else:
        pairs = [k for ka, _, kb, _ in S.PRODUCTS for k in (ka, kb) if k is not None]       # (product, operand it reads)
        n_ops = len(pairs)
        if variant == "swap_q":
            exempt = sum(1 for k in pairs if k in ((32,), (16,)))
        else:
            exempt = n_ops if P <= 32 else 0
        assert len(changes) == n_ops - exempt
    silent = [k for k, v in changes.items() if not v > 0]
    assert not silent, (P, variant, silent)
