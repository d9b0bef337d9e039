"""The integer probe's model against itself (tests/integer_probe_model.py; DESIGN.md "Integer probe"): the probe sets meet
the exactness conditions, two summation orders of the fp32 emulation equal the float64 value bit for bit, the sets reach
every weight position and bias slot, and planted faults change an output.  No point and no output is left out of any
comparison here.
"""
import functools

import numpy as np
import pytest

import integer_probe_model as M
from encoder_probe_model import round_to

VIEWS = {"fp32": "fp32", "bf16": "fp32", "fp16": "fp16"}           # operand type -> the kernel view of its weights


@pytest.fixture(scope="module")
def sets():
    return M.probe_sets()


@functools.lru_cache(maxsize=None)
def _bench(index, view):
    return M.FaultBench(M.probe_sets()[index], view)


def bench(ps, T):
    return _bench(ps.index, VIEWS[T])


def test_every_set_meets_the_conditions(sets):
    """exactness, run afresh, for every type a set is meant for; it returns what the set carries as expected output.  Every
    layer has a dense set for every type, and S is as DESIGN.md states it."""
    for ps in sets:
        for T in ps.types:
            out = M.exactness(ps.sd, M.universe(ps.zero).v, T)
            assert np.array_equal(out, ps.out), (ps, T)
    for T in M.TYPES:
        for L in range(11):
            for half in ((0, 1) if L == 8 else (None,)):
                parts = sorted(ps.part for ps in M.sets_for(T) if ps.L == L and ps.half == half)
                assert parts and parts == [(parts[0][0], p) for p in range(parts[0][0])], (T, L, half, parts)
        assert sorted(ps.zero for ps in M.sets_for(T) if ps.L is None) == [0, 1, 2]
    print("S per layer, bf16:", M.split_table(), "| sets:", len(sets), "| universe sizes:",
          [len(M.universe(z).v) for z in (None, 0, 1, 2)])
    assert all(S in (1, 2, 4) for S in M.split_table().values())


def test_split_supports_partition_the_matrix(sets):
    for L in range(11):
        for sel in ((0, 1) if L == 8 else (None,)):
            fam = [ps for ps in M.sets_for("bf16") if ps.L == L and ps.half == sel]
            key = M.LAYER_KEY[L] + ".weight"
            count = sum((ps.sd[key] != 0).int() for ps in fam).numpy()
            chain = count[:, :3] if L == 0 else count[:, :259] if L in (5, 9) else count
            assert (chain == 1).all(), (L, sel)


def test_representable_agrees_with_round_to():
    """The condition on operands is round_to's: a few values on both sides of the 8- and 11-bit limits."""
    vals = np.array([0.0, 0.25, 63.75, 64.25, 64.5, 255.0, 256.0, 257.0, 258.0, 511.75, 512.0, 2047.0, 2048.0, 2049.0, 2050.0])
    assert M.representable(vals, "bf16").tolist() == [v == round_to(v, "bf16") for v in vals]
    assert M.representable(vals, "bf16").tolist() == [True, True, True, False, True, True, True, False, True, False, True,
                                                      False, True, False, False]
    assert M.representable(vals, "fp16").tolist() == [True] * 13 + [False, True]


def test_conditions_are_not_vacuous(sets):
    """A set that breaks a condition is refused: a weight of 257 (bf16), an input of 1/8, the fp32 / fp16 layer-1 set in bf16."""
    ps = sets[0]
    v = M.universe(None).v
    sd = {k: t.clone() for k, t in ps.sd.items()}
    sd["color_fc.2.weight"][0, 0] = 257.0
    with pytest.raises(M.NotExact):
        M.exactness(sd, v, "bf16")
    M.exactness(sd, v, "fp16")
    v2 = v.copy()
    v2[0, 0] = 0.125
    with pytest.raises(M.NotExact):
        M.exactness(ps.sd, v2, "fp32")
    dense1 = next(p for p in M.sets_for("fp16") if p.L == 1)
    if "bf16" not in dense1.types:
        with pytest.raises(M.NotExact):
            M.exactness(dense1.sd, v, "bf16")


def test_two_summation_orders_equal_float64_bit_for_bit(sets):
    """Order independence: ascending k with the bias first, and a permuted k with the bias last, in fp32 on operands rounded
    to T, both equal the float64 forward at every point and output."""
    n = 0
    for ps in sets:
        want = ps.out.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), ps.out)
        for T in ps.types:
            for order in (None, 1 + ps.index):
                got = M.emulate(ps.sd, M.universe(ps.zero).v, T, order)
                assert got.dtype == np.float32 and np.array_equal(got, want), (ps, T, order, int((got != want).sum()))
                n += 1
    print(f"{n} emulated forwards equal float64")


def test_emulation_is_not_exact_on_ordinary_weights(synthetic):
    """The same emulation on dense random weights does depend on the order: the equality above is a property of the sets."""
    sd = synthetic.synthetic_state_dict(0, "structured")
    v = M.universe(None).v[:64]
    assert not np.array_equal(M.emulate(sd, v, "fp32", None), M.emulate(sd, v, "fp32", 3))


def _coverage(T):
    """Per layer of T's kernel view: weight positions that carry a nonzero weight on a nonzero activation in some set, weight
    positions that carry a nonzero weight at all, bias slots that are nonzero in some set."""
    live, nonzero, bias = {}, {}, {}
    for ps in M.sets_for(T):
        b = bench(ps, T)

        def visit(L, a, W, bb, y):
            act = (a != 0).any(0)
            live[L] = live.get(L, 0) | ((W != 0) & act[None, :])
            nonzero[L] = nonzero.get(L, 0) | (W != 0)
            bias[L] = bias.get(L, 0) | (bb != 0)
        M.layer_inputs_from(b.layers, b.v, visit=visit)
    return live, nonzero, bias


@pytest.mark.parametrize("T", M.TYPES)
def test_coverage(T):
    """Every (row, k) of every weight matrix as the kernel of type T reads it -- the sigma row, the folded colour layer (fp16)
    and both halves of color_fc.0's chain block included -- meets a nonzero activation with a nonzero weight at one point at
    least; every bias slot is nonzero in some set.  The sin columns cannot: sin is exact only where it is 0.  They carry a
    nonzero weight in the encoder sets and are covered by displacement (test_fault_classes: the sin / cos swap and the moved
    weight)."""
    live, nonzero, bias = _coverage(T)
    total = hit = 0
    for L in range(11):
        sin = np.zeros(live[L].shape[1], bool)
        if L in (0, 5, 9):
            base, levels = (0 if L == 0 else 256), (M.LD if L == 9 else M.LP)
            for c in range(3):
                sin[base + M.trig_cols(c, levels)[0::2]] = True
        assert live[L][:, ~sin].all(), (T, L, np.argwhere(~live[L][:, ~sin])[:5])
        assert not live[L][:, sin].any() and nonzero[L][:, sin].all(), (T, L)
        assert bias[L].all(), (T, L, np.flatnonzero(~bias[L])[:8])
        total += live[L].size
        hit += int(live[L].sum()) + int(nonzero[L][:, sin].sum())
    nb = sum(b.size for b in bias.values())
    print(f"{T}: {hit} of {total} weight positions covered ({sum(int(l[:, :].sum()) for l in live.values())} by value, the sin "
          f"columns by displacement), {nb} of {nb} bias slots")
    assert hit == total


def test_non_triviality(sets):
    """Behind a layer L < 8 under test the ReLU is live for 20-80 % of (point, unit) pairs; no output column is constant."""
    for ps in sets:
        assert (ps.out.max(0) > ps.out.min(0)).all(), ps
        if ps.L is not None and ps.L < 8:
            stats = {}
            M.exactness(ps.sd, M.universe(ps.zero).v, ps.types[0], stats)
            assert 0.2 <= stats[ps.L][1] <= 0.8, (ps, stats[ps.L])
            print(f"{ps.name}: live {stats[ps.L][1]:.2f}, largest input {max(s[0] for s in stats.values()):.0f} quanta")


def _dense_set(T, L, half=None):
    return next(ps for ps in M.sets_for(T) if ps.L == L and (half is None or ps.half == half))


def _selected_half(ps):
    """The half of h9 that the set's color_fc.0 reads (None: all of it, the layer-9 sets).  A row of layers_2 in the other
    half reaches no output of this set; the set of the other half observes it."""
    return None if ps.L == 9 else int(ps.sd["color_fc.0.weight"][0, 128] != 0)


def _enc_set(T, c):
    return next(ps for ps in M.sets_for(T) if ps.zero == c)


@pytest.mark.parametrize("T", M.TYPES)
def test_fault_classes(T):
    """Every class of planted fault, at every layer it applies to, changes an output of the set under test at that layer."""
    rng = np.random.Generator(np.random.PCG64(5))
    missed, n = [], 0

    def check(b, faulty, L, what):
        nonlocal n
        n += 1
        if not b.detected(faulty, L):
            missed.append((T, L, what))

    for L in range(11):
        half = int(rng.integers(2)) if L == 8 else None            # layers_2: the set that reads the half under the fault
        b = bench(_dense_set(T, L, half), T)
        W, bias = b.layers[L]
        rows, K = W.shape
        chain = 3 if L == 0 else 256 if L in (5, 9) else K
        seen = slice(128 * half, 128 * half + 128) if L == 8 and rows > 1 else slice(0, rows)
        r, k = (int(x) for x in rng.permutation(np.argwhere(W[seen, :chain - 1] != 0))[0])
        r += seen.start
        check(b, M.fault_move(b.layers, L, r, k), L, f"move ({r}, {k})")
        k = int(rng.choice(np.flatnonzero(np.abs(W[:, :chain]).sum(0))))
        check(b, M.fault_drop_column(b.layers, L, k), L, f"drop column {k}")
        k = int(rng.integers(0, chain - 1))
        check(b, M.fault_duplicate_column(b.layers, L, k), L, f"duplicate column {k}")
        if rows >= 32:
            t = int(rng.integers(seen.start // 16, seen.stop // 16 - 1))
            check(b, M.fault_bias_tile(b.layers, L, t), L, f"bias tile {t}")
        if L >= 1:
            t, q = int(rng.integers(seen.start // 16, (seen.stop + 15) // 16)), int(rng.integers(1, chain // 32))
            check(b, M.fault_fragment(b.layers, L, t, q), L, f"fragment ({t}, {q})")
    if T == "fp16":
        for ps in M.sets_for(T):                       # the folded bias has a term per (row, k) with Wc[r, k] b2[k] != 0
            Wc, b2 = ps.sd["color_fc.0.weight"].numpy()[:, :256], ps.sd["layers_2.bias"].numpy()
            terms = np.argwhere((Wc != 0) & (b2 != 0)[None, :])
            assert len(terms), ps
            r, k = (int(x) for x in terms[rng.integers(len(terms))])
            b = bench(ps, T)
            check(b, M.fault_folded_bias(b.layers, ps.sd, r, k), 9, f"folded bias term ({r}, {k}) of {ps.name}")
    for c in range(3):
        b = bench(_enc_set(T, c), T)
        for L in (0, 5, 9):
            for level in range(M.LD if L == 9 else M.LP):
                check(b, M.fault_swap_trig(b.layers, L, c, level), L, f"sin / cos swap, coordinate {c}, level {level}")
    print(f"{T}: {n} planted faults of every class, {len(missed)} undetected")
    assert not missed, missed


def test_single_position_fault_sample():
    """A seeded sample of single-position faults over all types, sets and layers: one weight multiplies the neighbouring
    input, or one weight is dropped (a weight on a sin column is always moved: dropping a factor of an exact zero changes
    nothing, by construction).  A fault in a row of layers_2 is drawn among the rows that the set's color_fc.0 reads (the
    other half belongs to the set of the other half).  At most 2 % may go undetected: those behind a ReLU that is dead at
    every point."""
    rng = np.random.Generator(np.random.PCG64(6))
    n, missed, per_layer = 0, [], np.zeros(11, int)
    for i in range(264):
        T = M.TYPES[i % 3]
        L = (i // 3) % 11
        cands = M.sets_for(T)
        ps = cands[rng.integers(len(cands))]
        b = bench(ps, T)
        W = b.layers[L][0]
        half = _selected_half(ps)
        seen = slice(128 * half, 128 * half + 128) if L == 8 and W.shape[0] > 1 and half is not None else slice(0, len(W))
        if seen.start or seen.stop < len(W):                       # the sigma row is read by every set
            seen = np.r_[seen, 256]
        r, k = (int(x) for x in rng.permutation(np.argwhere(W[seen] != 0))[0])
        r = int(np.arange(len(W))[seen][r])
        sin = ps.zero is not None and L in (0, 5, 9) and k >= (0 if L == 0 else 256) + 3 and (k - (0 if L == 0 else 256) - 3) % 2 == 0
        if sin or (rng.integers(2) and W.shape[1] > 1):
            faulty, what = M.fault_move(b.layers, L, r, k, 1 if k + 1 < W.shape[1] else -1), "move"
        else:
            faulty, what = M.fault_zero(b.layers, L, r, k), "drop"
        n += 1
        per_layer[L] += 1
        if not b.detected(faulty, L):
            missed.append((T, ps.name, L, what, r, k))
    print(f"{n} single-position faults ({per_layer.tolist()} per layer), {len(missed)} undetected: {missed}")
    assert n >= 200 and per_layer.min() >= 18
    assert len(missed) <= 0.02 * n, missed
