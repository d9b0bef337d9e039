"""CPU model behind the encoder probe (tests/test_encoder_probe_cpu.py, tests/test_gpu_encoder_probe.py; DESIGN.md "Encoder
probe"): every positional-encoder feature that the fused kernels form in registers, observed one column at a time and
compared with float64.

The fused 16-bit kernels encode with the hardware sine on an argument in revolutions (csrc/nerf_device.h: to_revolutions +
enc_lane; sincos_rev_fast in the stored bf16 rows of csrc/encode.hip).  Nothing of that is an output.  The probe makes it
one:

  probe weight sets   state dicts of the default Nerf() that are zero except one-hot taps.  A tap of encoder column j takes
        two hidden units, +col_j and -col_j, every later 256x256 layer is the identity on those two units, and the head
        reads unit_a - unit_b = relu(f) - relu(-f) = f.  The readout is exact in the operand type: the feature is rounded
        ONCE, when it becomes an MFMA operand; a product with 1, a sum with zeros and a second rounding to the same type
        change nothing, and the fp16 fold Wc[:, :256] W2 of two identities is an identity.  Four taps per set (sigma and
        the three colour channels) through three entry points: the posx columns into layers_0.0 ("l0") and into
        skip_conn_layer.0 ("skip"), the posd columns into color_fc.0 ("posd").
  ref_feature         float64 sin / cos of 2^l float64(x_fp32) in the reference's column order (raw coordinates first, then
        [sin, cos] per level per coordinate); raw columns are x itself.
  interval_check      in place of a tolerance on rounded values: for the operand type T and a phase allowance E, got passes
        iff round_T(ref - E) <= got <= round_T(ref + E).  The excess (distance from ref to the set of reals that round to
        got, 0 inside it) is what the readout can say about the encoder's own error: its maximum over a sweep is the measured
        error.  The readout is sharp only where the feature is tiny -- half an ulp of T at |f| ~ 1 is 2^-9 (bf16) or 2^-12
        (fp16) -- so the sweep sits on the zero crossings of every (level, trig) and SHARP_MIN of them must have a half-ulp
        of at most SHARP_HALF_ULP.
  emulate_fast_encoder   the kernels' fp32 phase arithmetic, rounding for rounding, with a float64 sine in place of the
        hardware one: bounds the arithmetic part of the error (ARITH_BOUND) and feeds the planted faults of the CPU test.

Constants: ENC_ATOL is the exact encoder's bound of tests/test_gpu_parity.py (the fp32 kernel uses sinf / cosf);  E_CAP = 2e-6
is the figure tests/test_gpu_training.py::test_sample_encode_bf16_matches_fp32_encoder already commits to; E_FAST is what
the GPU test asserts, derived from the measured maximum (see there).
"""
import functools

import numpy as np
import torch

from nerf_simple_amd.utils.synthetic import PARAM_SPECS

LP, LD = 10, 4
ENTRIES = {"l0": (63, LP), "skip": (63, LP), "posd": (27, LD)}      # entry point -> (columns, levels)
SIGMA = 3                                                            # output channel of sigma; 0..2 are r, g, b

ENC_ATOL = 5e-7            # tests/test_gpu_parity.py: ocml sinf / cosf on the exactly scaled argument
E_CAP = 2e-6               # the project's stated total for the hardware-trig encoder
ARITH_BOUND = 6e-7         # phase arithmetic alone against float64 (test_emulated_phase_arithmetic prints the measured value)
# Asserted allowances, |x| <= VERIFIED_LIM: twice the largest excess measured on the GPU over all sweeps and kernel paths,
# rounded up to one significant digit, where that is below the cap (tests/test_gpu_encoder_probe.py prints the maxima;
# table in DESIGN.md "Encoder probe").
#   enc_lane (in-register features of every fused 16-bit kernel): measured 5.58e-7 (fp16 readout of the cos lanes), twice
#     that is 1.12e-6, which rounds up to 2e-6: the cap itself;
#   sincos_rev_fast (stored bf16 rows of csrc/encode.hip): measured 3.74e-7, twice that is 7.5e-7 -> 8e-7.
E_FAST = 2e-6
E_ROWS = 8e-7
VERIFIED_LIM = 4096.0
SHARP_HALF_ULP = 2.5e-7
SHARP_MIN = 64
SHARP_REF = {"bf16": 6.4e-5, "fp16": 5e-4}                           # |ref| with half an ulp of T <= SHARP_HALF_ULP

# operand types: significand bits (hidden one included), exponent of the smallest normal, largest finite value
_TYPES = {"fp16": (11, -14, 65504.0), "bf16": (8, -126, float(np.float32(3.3895313892515355e38)))}
FP16_MIN_NORMAL = 2.0 ** -14
# Does the fp16 MFMA operand path flush subnormals (|f| < 2^-14)?  Measured by test_gpu_encoder_probe.py::
# test_fp16_subnormal_operands; when True the interval check falls back to |got - ref| <= 2^-14 on those elements.
FP16_OPERANDS_FLUSH = False


# ---- columns ----------------------------------------------------------------------------------------------------------
def column_info(entry, column):
    """(coordinate 0..2, level, trig) of a column of an entry point; level = -1 for the raw coordinates (trig 0 = sin)."""
    ncol, L = ENTRIES[entry]
    assert 0 <= column < ncol
    if column < 3:
        return column, -1, 0
    c, r = divmod(column - 3, 2 * L)
    return c, r // 2, r % 2


def ref_feature(v64, column, entry="l0"):
    """float64 reference of one encoder column: v64 [P, 3] = float64 of the fp32 position (or direction)."""
    c, level, trig = column_info(entry, column)
    x = np.asarray(v64, dtype=np.float64)[:, c]
    if level < 0:
        return x.copy()
    a = x * 2.0 ** level                         # exact: a power-of-two product, as in the reference's fp32
    return np.cos(a) if trig else np.sin(a)


def ref_rows(v64, entry):
    """All columns of an entry point at once: [P, 63] / [P, 27]."""
    return np.stack([ref_feature(v64, j, entry) for j in range(ENTRIES[entry][0])], axis=1)


# ---- rounding to an operand type, from float64, one rounding ------------------------------------------------------------
def _quantum(x, T):
    p, emin, _ = _TYPES[T]
    _, e = np.frexp(np.abs(x))                    # |x| = m 2^e, m in [0.5, 1)
    e = np.where(x == 0, emin + 1, e)             # (frexp(0) says e = 0)
    return np.ldexp(1.0, np.maximum(e, emin + 1) - p)


def round_to(x, T):
    """Round-to-nearest-even of float64 x to fp16 / bf16 (subnormals kept, overflow to inf), returned as float64."""
    x = np.asarray(x, dtype=np.float64)
    q = _quantum(x, T)
    r = np.rint(x / q) * q                        # x / q is exact (a power of two), rint rounds half to even
    return np.where(np.abs(r) > _TYPES[T][2], np.copysign(np.inf, x), r)


def rounding_cell(got, T):
    """[lo, hi]: the reals that round to the T value `got` (ties included)."""
    got = np.asarray(got, dtype=np.float64)
    p, emin, _ = _TYPES[T]
    q = _quantum(got, T)
    m, e = np.frexp(np.abs(got))
    # towards zero from a power of two above the smallest normal the spacing halves
    q_in = np.where((m == 0.5) & (e > emin + 1), q / 2, q)
    a = np.abs(got)
    lo_abs, hi_abs = a - q_in / 2, a + q / 2
    lo = np.where(got > 0, lo_abs, np.where(got < 0, -hi_abs, -q / 2))
    hi = np.where(got > 0, hi_abs, np.where(got < 0, -lo_abs, q / 2))
    return lo, hi


def excess(got, ref, T):
    """Distance from ref to the rounding cell of got (0 inside): what a T readout proves about |value - ref|."""
    if T == "fp32":
        return np.abs(np.asarray(got, np.float64) - ref)
    lo, hi = rounding_cell(got, T)
    return np.maximum(0.0, np.maximum(lo - ref, ref - hi))


def interval_check(got, ref, T, E, fp16_flush=False):
    """(ok, excess) per element.  16-bit T: ok iff round_T(ref - E) <= got <= round_T(ref + E); E = 0 (raw columns) demands
    round_T(ref) exactly.  T = 'fp32': |got - ref| <= E.  fp16_flush: the elements with |ref| < 2^-14 (fp16 subnormals, which
    the MFMA operand path may flush) pass iff |got - ref| <= 2^-14."""
    got = np.asarray(got, dtype=np.float64)
    ex = excess(got, ref, T)
    if T == "fp32":
        return np.abs(got - ref) <= E, ex
    ok = (round_to(ref - E, T) <= got) & (got <= round_to(ref + E, T))
    if fp16_flush and T == "fp16":
        sub = np.abs(ref) < FP16_MIN_NORMAL
        ok = np.where(sub, np.abs(got - ref) <= FP16_MIN_NORMAL, ok)
        ex = np.where(sub, 0.0, ex)
    return ok, ex


# ---- the kernels' phase arithmetic ------------------------------------------------------------------------------------
_C_HI = np.float32(0.15915494)               # fl32(1 / (2 pi))        (csrc/nerf_device.h to_revolutions)
_C_LO = np.float32(6.4206382e-09)            # 1 / (2 pi) - C_HI


def to_revolutions(x):
    """x / (2 pi) as hi + lo, the kernel's roundings: hi = fl(x C_HI), err = fma(x, C_HI, -hi), lo = fma(x, C_LO, err)."""
    x = np.asarray(x, dtype=np.float32)
    hi = x * _C_HI
    x64 = x.astype(np.float64)
    err = (x64 * np.float64(_C_HI) - hi.astype(np.float64)).astype(np.float32)     # the product is exact in float64
    lo = (x64 * np.float64(_C_LO) + err.astype(np.float64)).astype(np.float32)
    return hi, lo


def fast_phase(x, level, trig, variant, drop_lo=False):
    """The fp32 argument, in revolutions, that the hardware sine (enc_lane) or sine / cosine (sincos_rev_fast) receives."""
    hi, lo = to_revolutions(x)
    sc = np.float32(2.0 ** level)
    t = hi * sc                                                   # exact
    fr = (t.astype(np.float64) - np.floor(t.astype(np.float64))).astype(np.float32)       # v_fract_f32
    f = fr if drop_lo else fr + lo * sc                            # lo * sc is exact: with or without contraction
    if variant == "enc_lane" and trig:
        f = f + np.float32(0.25)
    return f


def emulate_fast_encoder(v, column, variant, entry="l0", *, drop_lo=False, phase_error=0.0):
    """One column as the fast encoders form it, hardware sine replaced by float64: v [P, 3] fp32.  variant 'enc_lane'
    (sin of the phase + trig / 4) or 'sincos_rev_fast' (sin and cos of one phase).  drop_lo / phase_error (radians) plant
    the faults of the CPU test."""
    assert variant in ("enc_lane", "sincos_rev_fast")
    c, level, trig = column_info(entry, column)
    x = np.asarray(v, dtype=np.float32)[:, c]
    if level < 0:
        return x.astype(np.float64)
    a = 2.0 * np.pi * fast_phase(x, level, trig, variant, drop_lo).astype(np.float64) + phase_error
    return np.cos(a) if (trig and variant == "sincos_rev_fast") else np.sin(a)


# ---- the input sweep ----------------------------------------------------------------------------------------------------
_EPS = (0.0, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4)
# more offsets for a level with fewer than SHARP_MIN crossings: near pi / 2 the fp32 spacing is 1.2e-7, so the offsets
# eps / 2^level that the higher levels bring to such a crossing fall onto the same few fp32 numbers
_EPS_FEW = tuple(s * e for e in (2e-6, 3e-6, 5e-6, 7e-6, 2e-5, 3e-5, 5e-5) for s in (1, -1))
_M_PER_LEVEL = 256


def _crossings(level, trig, lim):
    """(zero crossings (m + trig / 2) pi / 2^level inside [-lim, lim] as float64, all of them?): beyond _M_PER_LEVEL of them
    an even spread is taken."""
    step = np.pi / 2.0 ** level
    m_hi = int(np.floor(lim / step - trig / 2.0))
    m_lo = -int(np.floor(lim / step + trig / 2.0))
    m = np.arange(m_lo, m_hi + 1)
    complete = len(m) <= _M_PER_LEVEL
    if not complete:
        m = np.unique(np.round(np.linspace(m_lo, m_hi, _M_PER_LEVEL)).astype(np.int64))
    return (m + trig / 2.0) * step, complete


def _level_crossings(lim, max_level):
    """{(level, trig): crossings}.  A crossing of a lower level, sin or cos, is a sin crossing of every higher one; where a
    level is thinned to _M_PER_LEVEL crossings those of the complete levels below are put back, so that the low levels --
    which have only a handful of crossings of their own -- are also visited with the fine offsets of the high ones."""
    out, coarse = {}, []
    for level in range(max_level + 1):
        both = [_crossings(level, trig, lim) for trig in (0, 1)]
        for trig, (z, complete) in enumerate(both):
            if trig == 0 and not complete and coarse:
                z = np.union1d(z, np.concatenate(coarse))
            out[(level, trig)] = z
        coarse += [z for z, complete in both if complete]
    return out


@functools.lru_cache(maxsize=None)
def sweep_values(lim, n_random=2048, max_level=LP - 1):
    """Deterministic fp32 sweep of one coordinate over [-lim, lim] (module docstring; the issue's recipe): crossings of every
    (level, trig) with offsets eps / 2^level, a uniform fill, edge values.  Unique values in a fixed shuffled order."""
    vals = []
    for (level, trig), z in _level_crossings(lim, max_level).items():
        for eps in _EPS + (_EPS_FEW if len(z) < SHARP_MIN else ()):
            vals.append((z + eps / 2.0 ** level).astype(np.float32))
    rng = np.random.Generator(np.random.PCG64(20))
    vals.append(rng.uniform(-lim, lim, n_random).astype(np.float32))
    tiny = np.float32(np.finfo(np.float32).tiny)
    edges = [0.0, -0.0, 1.0, -1.0, 4.5, -4.5, tiny, -tiny, np.float32(1e-41), np.float32(-1e-41), 1e-20, -1e-20]
    k = 0
    while 2.0 ** k <= lim:
        edges += [2.0 ** k, -(2.0 ** k), 2.0 ** -k]
        k += 1
    vals.append(np.asarray(edges, dtype=np.float32))
    # fl32(x / 2 pi) 2^level an integer: x = fl32(2 pi k / 2^j), where the product with C_HI rounds onto k / 2^j
    cand = (2.0 * np.pi * np.arange(1, 513) / 512.0 * min(1.0, lim / 6.3)).astype(np.float32)
    cand = np.concatenate([cand, (2.0 * np.pi * np.arange(-8, 9) / 8.0).astype(np.float32)])
    hi = cand * _C_HI
    vals.append(cand[(hi * np.float32(512.0)) == np.round(hi * np.float32(512.0))])
    v = np.concatenate(vals)
    v = v[np.abs(v) <= np.float32(lim)]
    # unique by bit pattern (keeps -0 next to +0), then a fixed shuffle so that a tile does not hold neighbours only
    _, idx = np.unique(v.view(np.uint32), return_index=True)
    v = v[np.sort(idx)]
    return np.ascontiguousarray(v[np.random.Generator(np.random.PCG64(21)).permutation(len(v))])


@functools.lru_cache(maxsize=None)
def sweep_points(lim):
    """[S, 6] fp32 query points: every column carries the whole sweep, each in an order of its own.  In points mode the
    kernels take columns 3..5 as they are (no normalisation), so the direction features see the full sweep as well."""
    s = sweep_values(lim)
    cols = [s] + [s[np.random.Generator(np.random.PCG64(30 + k)).permutation(len(s))] for k in range(1, 6)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


@functools.lru_cache(maxsize=None)
def sweep_directions(n):
    """[n, 3] fp32 DISTINCT directions, not normalised exactly (the kernels normalise): a component at each zero crossing of
    levels 0..3 inside (-1, 1) with the sweep's offsets, the other two components splitting the rest at a changing angle;
    first the six axes and near-degenerate ones."""
    special = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1),
               (1, 1e-7, -0.0), (-0.0, 1, 1e-7), (1e-7, -0.0, -1), (1, -1e-7, 1e-7)]
    comp = []
    for (level, trig), z in _level_crossings(0.999, LD - 1).items():
        for eps in _EPS:
            comp.append(z + eps / 2.0 ** level)
    comp = np.unique(np.concatenate(comp))
    comp = comp[np.random.Generator(np.random.PCG64(22)).permutation(len(comp))]
    out = [np.asarray(s, dtype=np.float64) for s in special]
    i = 0
    while len(out) < n:
        c = comp[i % len(comp)]
        axis = (i // len(comp) + i) % 3
        phi = 2.0 * np.pi * ((0.1 + i * 0.6180339887498949) % 1.0)
        r = np.sqrt(1.0 - c * c)
        d = np.empty(3)
        d[axis], d[(axis + 1) % 3], d[(axis + 2) % 3] = c, r * np.cos(phi), r * np.sin(phi)
        out.append(d)
        i += 1
    return np.ascontiguousarray(np.stack(out[:n]).astype(np.float32))


def probe_rays(B, N, lim=None):
    """rays [B, 6] and sorted sample positions ts [B, N] (fp32) for the rays-mode kernels: every ray has a direction of its
    own (sweep_directions, scaled off unit length so that the normalisation matters) and an origin of its own.  With `lim`
    the origins ARE the first B sweep points and ts = 0 (the kernel then forms x = origin: the value sweep, N = 1)."""
    d = sweep_directions(B).astype(np.float64)
    rng = np.random.Generator(np.random.PCG64(1000 * B + N))
    if lim is not None:
        o = sweep_points(lim)[:B, :3].astype(np.float64)
        ts = np.zeros((B, N))
    else:
        unit = d / np.linalg.norm(d, axis=1, keepdims=True)
        o = -4.0 * unit + rng.uniform(-0.25, 0.25, (B, 3))
        ts = np.sort(rng.uniform(2.0, 6.0, (B, N)), axis=1)
    d = d * rng.uniform(0.75, 1.25, (B, 1))
    return np.ascontiguousarray(np.concatenate([o, d], axis=1).astype(np.float32)), np.ascontiguousarray(ts.astype(np.float32))


def sharp_counts(lim, T, entry="l0", lo=0.0):
    """{(level, trig): sweep values whose reference feature has lo <= |ref| <= SHARP_REF[T]} for an entry point's levels."""
    x = sweep_values(lim).astype(np.float64)
    out = {}
    for level in range(ENTRIES[entry][1]):
        for trig in (0, 1):
            ref = np.abs(np.cos(x * 2.0 ** level) if trig else np.sin(x * 2.0 ** level))
            out[(level, trig)] = int(((ref >= lo) & (ref <= SHARP_REF[T])).sum())
    return out


# ---- probe weight sets ----------------------------------------------------------------------------------------------------
def probe_state_dict(taps, unit0=0):
    """State dict of Nerf() (10, 4, 256), all zero but the taps [(output channel, entry, column), ...] (at most one per output
    channel; sigma takes 'l0' / 'skip' only).  Tap k lives on hidden units unit0 + 2k, + 1 (unit0 even)."""
    assert unit0 % 2 == 0 and len({t[0] for t in taps}) == len(taps) <= 4
    sd = {k: torch.zeros(shape, dtype=torch.float32) for k, shape in PARAM_SPECS}
    for k, (ch, entry, col) in enumerate(taps):
        assert 0 <= col < ENTRIES[entry][0]
        a = (unit0 + 2 * k) % 256
        b = a + 1
        ca = (unit0 + 2 * k) % 128
        cb = ca + 1
        if entry in ("l0", "skip"):
            if entry == "l0":
                sd["layers_0.0.weight"][a, col], sd["layers_0.0.weight"][b, col] = 1.0, -1.0
                for i in (2, 4, 6, 8):
                    sd[f"layers_0.{i}.weight"][a, a] = sd[f"layers_0.{i}.weight"][b, b] = 1.0
                sd["skip_conn_layer.0.weight"][a, a] = sd["skip_conn_layer.0.weight"][b, b] = 1.0
            else:
                sd["skip_conn_layer.0.weight"][a, 256 + col], sd["skip_conn_layer.0.weight"][b, 256 + col] = 1.0, -1.0
            for i in (0, 2):
                sd[f"layers_1.{i}.weight"][a, a] = sd[f"layers_1.{i}.weight"][b, b] = 1.0
            if ch == SIGMA:
                sd["sigma_fc.0.weight"][0, a], sd["sigma_fc.0.weight"][0, b] = 1.0, -1.0
                continue
            sd["layers_2.weight"][a, a] = sd["layers_2.weight"][b, b] = 1.0
            sd["color_fc.0.weight"][ca, a] = sd["color_fc.0.weight"][cb, b] = 1.0
        else:
            assert ch != SIGMA, "sigma does not depend on the direction"
            sd["color_fc.0.weight"][ca, 256 + col], sd["color_fc.0.weight"][cb, 256 + col] = 1.0, -1.0
        sd["color_fc.2.weight"][ch, ca], sd["color_fc.2.weight"][ch, cb] = 1.0, -1.0
    return sd


def all_taps():
    return [(e, j) for e in ("l0", "skip", "posd") for j in range(ENTRIES[e][0])]


def probe_tap_lists(sigma_only=False):
    """The taps of every weight set.  Default: all 153 (entry, column) pairs once, four per set (39 sets): sigma carries every
    third posx tap, the colour channels the rest with the posd taps spread among them.  sigma_only: the 126 posx taps, one
    per set, on sigma (the sigma-only kernel has no other output)."""
    posx = [(e, j) for e in ("l0", "skip") for j in range(63)]
    posd = [("posd", j) for j in range(27)]
    if sigma_only:
        return [[(SIGMA, e, j)] for e, j in posx]
    on_sigma = [t for i, t in enumerate(posx) if i % 3 == 0 and i < 117]          # 39
    rest = [t for t in posx if t not in on_sigma]                                  # 87
    colour = []
    while rest or posd:
        if posd and (len(colour) % 4 == 3 or not rest):
            colour.append(posd.pop(0))
        else:
            colour.append(rest.pop(0))
    sets = []
    for s, (e, j) in enumerate(on_sigma):
        taps = [(SIGMA, e, j)] + [(ch, *colour[3 * s + ch]) for ch in range(3) if 3 * s + ch < len(colour)]
        sets.append(taps)
    assert len(colour) <= 3 * len(sets)
    return sets


def probe_weight_sets(sigma_only=False):
    """Yields (state_dict, [(output channel, entry, column), ...]); the hidden units move from set to set."""
    for s, taps in enumerate(probe_tap_lists(sigma_only)):
        yield probe_state_dict(taps, unit0=(38 * s) % 256), taps
