"""CPU tests of the encoder probe's model (tests/encoder_probe_model.py): the probe weight sets isolate single encoder columns
of the reference network, the emulated phase arithmetic of the fast encoders stays within ARITH_BOUND of float64, the
committed sweep is sharp enough to see an error of the asserted size, and the interval check catches each planted fault."""
import numpy as np
import pytest
import torch

import encoder_probe_model as M


def test_rounding_helpers_against_the_library_types():
    """round_to / rounding_cell against numpy's fp16 and torch's bf16 on fp32 inputs (one rounding in both), subnormals and
    powers of two included."""
    rng = np.random.Generator(np.random.PCG64(0))
    x = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.uniform(-9, 4, 20000), 2.0 ** np.arange(-30.0, 15.0),
                        -(2.0 ** np.arange(-30.0, 15.0)), [0.0, 6e-8, 3e-8, 2.98e-8, 65504.0, 65519.0, 65520.0, 1e5]]).astype(np.float32)
    with np.errstate(over="ignore"):
        want16 = x.astype(np.float16).astype(np.float64)
    assert np.array_equal(M.round_to(x, "fp16"), want16)
    wantb = torch.from_numpy(x).to(torch.bfloat16).double().numpy()
    assert np.array_equal(M.round_to(x, "bf16"), wantb)
    for T, want in (("fp16", want16), ("bf16", wantb)):
        fin = np.isfinite(want)
        lo, hi = M.rounding_cell(want[fin], T)
        x64 = x[fin].astype(np.float64)
        assert np.all((lo <= x64) & (x64 <= hi))                       # a value lies in the cell of what it rounds to
        assert np.array_equal(M.round_to(lo + (hi - lo) * 0.25, T), want[fin])
        assert np.array_equal(M.round_to(lo + (hi - lo) * 0.75, T), want[fin])
        assert np.all(M.round_to(np.nextafter(hi, np.inf), T) > want[fin])
        assert np.all(M.round_to(np.nextafter(lo, -np.inf), T) < want[fin])
        assert not M.excess(want[fin], x64, T).any()


def test_tap_lists_cover_every_column_once():
    sets = M.probe_tap_lists()
    flat = [(e, j) for taps in sets for _, e, j in taps]
    assert len(sets) == 39 and sorted(flat) == sorted(M.all_taps()) and len(flat) == 153
    for taps in sets:
        chans = [ch for ch, _, _ in taps]
        assert len(set(chans)) == len(chans) and all(e != "posd" for ch, e, _ in taps if ch == M.SIGMA)
    # both posx entries reach colour channels as well as sigma
    assert {(e, ch == M.SIGMA) for taps in sets for ch, e, _ in taps} == {("l0", True), ("l0", False), ("skip", True),
                                                                          ("skip", False), ("posd", False)}
    sig = M.probe_tap_lists(sigma_only=True)
    assert sorted((e, j) for (ch, e, j), in sig) == sorted(t for t in M.all_taps() if t[0] != "posd")
    assert all(ch == M.SIGMA for (ch, _, _), in sig)


@pytest.mark.parametrize("sigma_only", [False, True], ids=["four-taps", "sigma-only"])
def test_probe_isolates_single_columns_of_the_reference(oracle, sigma_only):
    """Every probe weight set through the reference network (oracle.nerf_forward) on a few hundred sweep points: a tapped
    output EQUALS the reference encoder's column, an untapped one is exactly 0.  Pins the column order of the three entry
    points, the cat order [h ; x] of the skip and [h ; d] of the colour layer included."""
    v = torch.from_numpy(M.sweep_points(4.5)[:320].copy())
    posx, posd = oracle.positional_encoder(v)
    n = 0
    for sd, taps in M.probe_weight_sets(sigma_only):
        with torch.no_grad():
            out = oracle.nerf_forward(sd, v)
        tapped = {ch: (e, j) for ch, e, j in taps}
        for ch in range(4):
            if ch in tapped:
                e, j = tapped[ch]
                want = (posd if e == "posd" else posx)[:, j]
                assert torch.equal(out[:, ch], want), (taps, ch)
                n += 1
            else:
                assert not out[:, ch].any(), (taps, ch)
    assert n == (126 if sigma_only else 153)


def test_reference_columns_are_the_reference_encoders():
    """ref_feature in float64 against the reference encoder's fp32 columns: the same column order, within fp32 rounding."""
    import nerf_oracle as O
    v = M.sweep_points(4.5)[:500]
    posx, posd = O.positional_encoder(torch.from_numpy(v.copy()))
    assert np.abs(M.ref_rows(v[:, :3].astype(np.float64), "l0") - posx.numpy()).max() <= 1.2e-7
    assert np.abs(M.ref_rows(v[:, 3:].astype(np.float64), "posd") - posd.numpy()).max() <= 1.2e-7
    assert M.column_info("skip", 3 + 20 + 2 * 7 + 1) == (1, 7, 1) and M.column_info("posd", 3 + 16 + 5) == (2, 2, 1)


@pytest.mark.parametrize("lim", [4.5, 64.0, 4096.0])
def test_emulated_phase_arithmetic(lim):
    """to_revolutions + fract + lo * 2^l (+ 0.25 on enc_lane's cos lanes) in the kernels' fp32, float64 sine: within 6e-7 of
    float64 sin / cos (2^l x) at every level for |x| up to 4096.  Measured: 5.61e-7 (enc_lane, cos lanes: + 0.25 carries the
    sum past 1, where the ulp doubles) and 3.75e-7 (sincos_rev_fast) at each of the three limits."""
    v = M.sweep_points(lim)[:, :3]
    v64 = v.astype(np.float64)
    for variant in ("enc_lane", "sincos_rev_fast"):
        worst = {}
        for j in range(3, 63):
            _, level, trig = M.column_info("l0", j)
            err = np.abs(M.emulate_fast_encoder(v, j, variant) - M.ref_feature(v64, j)).max()
            worst[(level, trig)] = max(worst.get((level, trig), 0.0), float(err))
        print(f"lim {lim:g} {variant}: max |emulated - float64| = {max(worst.values()):.3e} "
              f"(sin {max(e for (l, t), e in worst.items() if not t):.3e}, cos {max(e for (l, t), e in worst.items() if t):.3e})")
        assert max(worst.values()) <= M.ARITH_BOUND
        for j in range(3):
            assert np.array_equal(M.emulate_fast_encoder(v, j, variant), v64[:, j])


def test_sweep_is_deterministic_and_sharp():
    """At lim = 4.5 every (level, trig) has at least SHARP_MIN sweep values whose reference feature has half an ulp of the
    operand type of at most 2.5e-7 (|ref| <= 6.4e-5 in bf16, <= 5e-4 in fp16), also when fp16 subnormals are left out.  At
    lim = 4096 this is not attainable for the top levels (the fp32 spacing 2.4e-4 times 2^9 is far above it): not required."""
    M.sweep_values.cache_clear()
    a = M.sweep_values(4.5).copy()
    M.sweep_values.cache_clear()
    assert np.array_equal(a.view(np.uint32), M.sweep_values(4.5).view(np.uint32))
    assert len(np.unique(a.view(np.uint32))) == len(a) and np.abs(a).max() <= 4.5
    for edge in (0.0, 1.0, 4.5, np.finfo(np.float32).tiny, np.float32(1e-41), np.float32(1e-20), 4.0):
        assert (a == np.float32(edge)).any() and (a == -np.float32(edge)).any(), edge
    assert (np.signbit(a) & (a == 0)).any()
    for lim in (64.0, 4096.0):
        s = M.sweep_values(lim)
        assert np.abs(s).max() <= lim and (s == lim).any() and np.abs(s).max() > 0.99 * lim
    for T in ("bf16", "fp16"):
        for entry in ("l0", "posd"):
            counts = M.sharp_counts(4.5, T, entry)
            poorest = min(counts, key=counts.get)
            print(f"{T} {entry}: poorest (level, trig) = {poorest} with {counts[poorest]} sharp points")
            assert counts[poorest] >= M.SHARP_MIN
    sharp16 = M.sharp_counts(4.5, "fp16", lo=M.FP16_MIN_NORMAL)
    print("fp16 without subnormal references: poorest", min(sharp16.values()))
    pts = M.sweep_points(4.5)
    for c in range(1, 6):
        assert np.array_equal(np.sort(pts[:, c].view(np.uint32)), np.sort(a.view(np.uint32)))
    d = M.sweep_directions(4096)
    assert len(np.unique(d, axis=0)) == 4096
    rays, ts = M.probe_rays(20, 40)
    assert len(np.unique(rays[:, 3:], axis=0)) == 20 and np.all(np.diff(ts, axis=1) >= 0)


# ---- planted faults ---------------------------------------------------------------------------------------------------------
def _check(got, ref, T, raw):
    ok, ex = M.interval_check(M.round_to(got, T), ref, T, 0.0 if raw else M.E_FAST)
    return bool(ok.all()), float(ex.max())


@pytest.mark.parametrize("T", ["bf16", "fp16"])
@pytest.mark.parametrize("variant", ["enc_lane", "sincos_rev_fast"])
def test_interval_check_passes_the_emulation_and_fails_each_planted_fault(T, variant):
    """The interval check at the asserted allowance E_FAST, fed the emulated encoder rounded once to the operand type: passes
    as it is and fails with each single defect."""
    v = M.sweep_points(4.5)
    x, d = v[:, :3], v[:, 3:]
    x64, d64 = x.astype(np.float64), d.astype(np.float64)

    def column(j, entry="l0", src=x, **kw):
        return M.emulate_fast_encoder(src, j, variant, entry, **kw)

    def ref(j, entry="l0", src64=x64):
        return M.ref_feature(src64, j, entry)

    # no defect: every column of every entry point passes, and the excess stays at the arithmetic bound
    worst = 0.0
    for entry, src, src64 in (("l0", x, x64), ("posd", d, d64)):
        for j in range(M.ENTRIES[entry][0]):
            ok, ex = _check(column(j, entry, src), ref(j, entry, src64), T, j < 3)
            assert ok, (entry, j)
            worst = max(worst, ex)
    print(f"{T} {variant}: max excess of the clean emulation {worst:.3e}")
    assert worst <= M.ARITH_BOUND

    def caught(make, cols=range(3, 63)):
        return [j for j in cols if not _check(make(j), ref(j), T, j < 3)[0]]

    # 1. a phase error of 4e-6 rad: every (level, trig) has sharp points, so every column sees it
    assert caught(lambda j: column(j, phase_error=4e-6)) == list(range(3, 63))
    # 2. q.lo dropped: 2 pi 2^l lo, up to ~1e-4 at level 9 -- the high levels see it (level 0 stays inside the allowance)
    lost = caught(lambda j: column(j, drop_lo=True))
    assert lost and {M.column_info("l0", j)[1] for j in lost} >= {5, 6, 7, 8, 9}, lost
    # 3. sin / cos swapped on one column; 4. level l taken as l + 1; 5. y read for z
    j = 3 + 20 * 1 + 2 * 3                                                             # y, level 3, sin
    assert not _check(column(j + 1), ref(j), T, False)[0]
    assert not _check(column(j + 2), ref(j), T, False)[0]
    jz = 3 + 20 * 2 + 2 * 3
    assert not _check(column(j), ref(jz), T, False)[0]
    # ... also on the lowest and the highest level, where neighbouring columns are most / least alike
    for level in (0, 8):
        j = 3 + 2 * level
        assert not _check(column(j + 1), ref(j), T, False)[0] and not _check(column(j + 2), ref(j), T, False)[0]
    # 6. a direction feature taken from the neighbouring ray: distinct directions per ray
    rays, _ = M.probe_rays(300, 1)
    dirs = rays[:, 3:].astype(np.float64)
    unit = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    for jd in range(27):
        good = column(jd, "posd", unit)
        assert _check(good, ref(jd, "posd", unit.astype(np.float64)), T, jd < 3)[0]
        assert not _check(np.roll(good, 1), ref(jd, "posd", unit.astype(np.float64)), T, jd < 3)[0], jd
    # 7. a raw column rounded twice (through three more bits first): caught by E = 0, invisible to any tolerance
    p = M._TYPES[T][0]
    x0 = x64[:, 0]
    _, e = np.frexp(np.abs(x0))
    q = np.ldexp(1.0, e - (p + 3))
    twice = M.round_to(np.rint(x0 / q) * q, T)
    assert np.all(np.abs(twice - M.round_to(x0, T)) <= M._quantum(x0, T))                   # one step at the most ...
    assert not M.interval_check(twice, x0, T, 0.0)[0].all()                                  # ... and still caught


def test_fp32_check_and_flush_rule():
    ref = np.array([0.0, 0.5, -1.0, 3e-5])
    ok, ex = M.interval_check(ref + np.array([0.0, 4e-7, -6e-7, 0.0]), ref, "fp32", M.ENC_ATOL)
    assert ok.tolist() == [True, True, False, True] and abs(ex[2] - 6e-7) < 1e-12
    # an fp16 subnormal flushed to zero: outside the interval, inside the flush rule, which touches only |ref| < 2^-14
    ok, _ = M.interval_check(np.array([0.0, 0.0]), np.array([3e-5, 7e-5]), "fp16", M.E_FAST)
    assert ok.tolist() == [False, False]
    ok, _ = M.interval_check(np.array([0.0, 0.0]), np.array([3e-5, 7e-5]), "fp16", M.E_FAST, fp16_flush=True)
    assert ok.tolist() == [True, False]
