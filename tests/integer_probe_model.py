"""CPU model behind the integer probe (tests/test_integer_probe_cpu.py, tests/test_gpu_integer_probe.py; DESIGN.md "Integer
probe"): weights and inputs for which the inference network kernels have exactly one right answer.

The inference kernels (csrc/mlp16_chain.h as instantiated by mlp_bf16_16.hip for fp16 / bf16, the sigma-only plan of
density.hip, the exact-f32 kernel mlp_f32.hip) keep their activations in registers; only four numbers per point come out.
Dense random weights can judge those four numbers by a tolerance only.  Here every weight, every bias and every
activation is a small multiple of one quantum (QUANTUM = 1/4; integers in points mode), exactly representable in the
operand type, and every dot product stays below 2^24 quanta even if all its terms had one sign: every partial sum of every
summation order is then an exact fp32 number, so a correct kernel returns the float64 value bit for bit and the tests
compare with np.array_equal.

  probe sets     state dicts of the default Nerf().  Internal layers as in csrc/nerf_layout.h: 0 = layers_0.0, 1..4 =
        layers_0.2..8, 5 = skip_conn_layer.0, 6..7 = layers_1, 8 = layers_2 + the sigma_fc.0 row, 9 = color_fc.0, 10 =
        color_fc.2.  One family per layer L under test: L dense in {-1, +1} (on its chain columns and its raw-coordinate
        columns) with integer biases; every other 256-wide layer the identity plus a sparse bias in {0, 1} (exact behind
        a ReLU: activations are >= 0), the skip layer [I | 0], color_fc.0 a selection of one half of h9 (the half alternates
        from set to set; the layer-8 family has one set per half), the sigma row and color_fc.2 dense +-1 read-outs, layer
        0 a {-1, 0, 1} combination of the three raw coordinates with a negative bias.  Where a dense layer does not meet the
        conditions below in bf16 it is split into S = 2 or 4 sets whose supports partition the matrix; the model takes the
        smallest S, bias shift and seed that pass (_family).
  encoder sets   one per coordinate c: dense +-1 on the sin / cos columns of coordinate c of layers 0 and 5 (position) and of
        layer 9 (direction), evaluated where x_c = 0 and d_c = 0: there sin = 0 and cos = 1 exactly, in float64 and in the
        kernels (the phase of 0 is 0).  A sin weight multiplies an exact zero: it is observed by displacement (a sin / cos
        swap, a shifted column), not by its value.
  inputs         probe_points: integer x in [-2, 2]^3, d in {-1, 0, 1}^3.  probe_rays: origins c - 4 d with integer c in
        [-1, 1]^3 and an axis-aligned unit d, bins over [2, 6] with N = 4 or 8 and jitter u in {0, 1/2}: ts and o + t d are multiples of 1/4.
        Both are fixed base batches that the GPU test tiles to any size, so that the conditions are checked on every input a
        kernel ever sees (universe).
  exactness      asserts, for an operand type T, (a) every weight as the kernel reads it -- for fp16 the folded colour layer
        Wc[:, :256] W2 with bias bc + Wc[:, :256] b2 -- is representable in T, (b) every layer input that meets a nonzero
        weight is, (c) sum |terms| + |bias| < 2^24 quanta for every dot product; returns the float64 outputs.
  emulate        the fp32 forward with operands rounded to T, summed in ascending or permuted k order (CPU test only).
  faults         planted on the weights as a kernel sees them (kernel_layers).
"""
import functools

import numpy as np
import torch

from encoder_probe_model import round_to
from nerf_simple_amd.utils.synthetic import PARAM_SPECS

TYPES = ("fp32", "bf16", "fp16")
QUANTUM = 0.25
LIMIT = 2.0 ** 24 * QUANTUM
LAYER_KEY = {0: "layers_0.0", 1: "layers_0.2", 2: "layers_0.4", 3: "layers_0.6", 4: "layers_0.8", 5: "skip_conn_layer.0",
             6: "layers_1.0", 7: "layers_1.2", 8: "layers_2", 9: "color_fc.0", 10: "color_fc.2"}
SIGMA_KEY = "sigma_fc.0"
LP, LD = 10, 4
BASE_POINTS = 499             # base batch sizes: primes, so that a tiled batch meets the kernels' tiles at every phase
BASE_RAYS = 509
RAY_N = (4, 8)
BIAS_EVERY = 8                # an identity layer's bias slot is nonzero in the sets of one family in BIAS_EVERY consecutive ones


def trig_cols(c, L):
    """Columns of the sin / cos features of coordinate c inside an encoder block of L levels: [sin_0, cos_0, sin_1, ...]."""
    return 3 + 2 * L * c + np.arange(2 * L)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probe_points(zero=None):
    """[BASE_POINTS, 6] fp32: integer x in [-2, 2]^3 (each of the 125 about four times), d in {-1, 0, 1}^3.  zero = c:
    x_c = 0 and d_c = 0 (encoder sets)."""
    rng = np.random.Generator(np.random.PCG64(100))
    g = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    x = g[np.arange(BASE_POINTS) % 125]
    d = rng.integers(-1, 2, (BASE_POINTS, 3))
    v = np.concatenate([x, d], 1).astype(np.float32)
    v = v[rng.permutation(BASE_POINTS)]
    if zero is not None:
        v[:, zero] = 0.0
        v[:, 3 + zero] = 0.0
    return np.ascontiguousarray(v)


@functools.lru_cache(maxsize=None)
def probe_rays(N, zero=None):
    """(rays [BASE_RAYS, 6], tb [N + 1], u [BASE_RAYS, N]) fp32.  d = +-e_axis, o = c - 4 d with integer c in [-1, 1]^3; zero = c: axis != c and c_c = 0, so that x_c = 0 and d_c = 0 at every sample."""
    rng = np.random.Generator(np.random.PCG64(200 + N))
    axes = [a for a in range(3) if a != zero]
    axis = np.asarray(axes)[rng.integers(0, len(axes), BASE_RAYS)]
    sign = rng.integers(0, 2, BASE_RAYS) * 2 - 1
    c = rng.integers(-1, 2, (BASE_RAYS, 3))
    if zero is not None:
        c[:, zero] = 0
    d = np.zeros((BASE_RAYS, 3))
    d[np.arange(BASE_RAYS), axis] = sign
    rays = np.concatenate([c - 4.0 * d, d], 1).astype(np.float32)
    tb = np.linspace(2.0, 6.0, N + 1).astype(np.float32)
    u = (rng.integers(0, 2, (BASE_RAYS, N)) * 0.5).astype(np.float32)
    return np.ascontiguousarray(rays), tb, np.ascontiguousarray(u)


def ray_samples(rays, tb, u):
    """float64 (ts [B, N], query points [B N, 6]) of the reference's sampling: ts = (tb[1] - tb[0]) u + tb[:-1], x = o + t d,
    the direction normalised (exact here: |d| = 1)."""
    rays, tb, u = (np.asarray(a, dtype=np.float64) for a in (rays, tb, u))
    ts = (tb[1] - tb[0]) * u + tb[:-1]
    o, d = rays[:, None, :3], rays[:, None, 3:]
    dn = d / np.linalg.norm(d, axis=2, keepdims=True)
    q = np.concatenate([o + d * ts[:, :, None], np.broadcast_to(dn, (len(rays), ts.shape[1], 3))], 2)
    return ts, q.reshape(-1, 6)


class Universe:
    """Every distinct input point of one `zero` class: v [U, 6] float64, and the rows of the base batches inside it."""

    def __init__(self, zero):
        pts = probe_points(zero).astype(np.float64)
        parts, self.ts = [pts], {}
        for N in RAY_N:
            self.ts[N], q = ray_samples(*probe_rays(N, zero))
            parts.append(q)
        self.v, inv = np.unique(np.concatenate(parts), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        self.points = inv[:len(pts)]
        self.rays, at = {}, len(pts)
        for N, q in zip(RAY_N, parts[1:]):
            self.rays[N] = inv[at:at + len(q)]
            at += len(q)


@functools.lru_cache(maxsize=None)
def universe(zero=None):
    return Universe(zero)


# ---- the network as a kernel sees it ----------------------------------------------------------------------------------------
def encode(x, L):
    """float64 encoder block [P, 3 + 6 L] in the reference's column order."""
    cols = [x]
    for c in range(3):
        for l in range(L):
            cols += [np.sin(2.0 ** l * x[:, c:c + 1]), np.cos(2.0 ** l * x[:, c:c + 1])]
    return np.concatenate(cols, 1)


def kernel_layers(sd, T):
    """[(W [rows, K], b [rows])] of the 11 internal layers in float64, source column order.  Unfolded (fp32, bf16): layer 8
    is [layers_2 ; sigma_fc.0] (257 rows).  Folded (fp16): layer 8 is the sigma row alone and layer 9 is
    [Wc[:, :256] W2 | Wc[:, 256:]] with bias bc + Wc[:, :256] b2, as csrc/nerf_layout.h fold_weight_at / fold_bias_at form them."""
    g = lambda k: sd[k].numpy().astype(np.float64)
    out = [[g(LAYER_KEY[L] + ".weight"), g(LAYER_KEY[L] + ".bias")] for L in range(11)]
    ws, bs = g(SIGMA_KEY + ".weight"), g(SIGMA_KEY + ".bias")
    if T == "fp16":
        W2, b2 = out[8]
        Wc, bc = out[9]
        out[9] = [np.concatenate([Wc[:, :256] @ W2, Wc[:, 256:]], 1), bc + Wc[:, :256] @ b2]
        out[8] = [ws, bs]
    else:
        out[8] = [np.concatenate([out[8][0], ws]), np.concatenate([out[8][1], bs])]
    return out


def layer_inputs_from(layers, v, start=0, h=None, visit=None, stop=10, sigma=None):
    """Runs layers[start:stop + 1] in float64 on points v [P, 6]; h = the chain input of layer `start` (None for 0), sigma
    [P, 1] = layer 8's last output where start > 8.  visit(L, a, W, b, y) sees every layer's full input a [P, K] and its
    output y before the activation.  Returns (out [P, 4] or None where stop < 10, {L: chain input of layer L})."""
    folded = layers[8][0].shape[0] == 1
    px, pd = encode(v[:, :3], LP), encode(v[:, 3:], LD)
    chain = {}
    for L in range(start, 11):
        chain[L] = h
        a = px if L == 0 else np.concatenate([h, px], 1) if L == 5 else np.concatenate([h, pd], 1) if L == 9 else h
        W, b = layers[L]
        y = a @ W.T + b
        if visit is not None:
            visit(L, a, W, b, y)
        if L == stop and L < 10:
            return None, chain
        if L == 8:
            sigma = y[:, -1:]
            h = h if folded else y[:, :256]
        elif L == 10:
            return np.concatenate([y, sigma], 1), chain
        else:
            h = np.maximum(y, 0.0)


def forward64(sd, v, T="fp32"):
    return layer_inputs_from(kernel_layers(sd, T), np.asarray(v, np.float64))[0]


def representable(a, T):
    """Elementwise: is the float64 value a T number?"""
    a = np.asarray(a, dtype=np.float64)
    if T == "fp32":
        return a.astype(np.float32).astype(np.float64) == a
    return round_to(a, T) == a


class NotExact(AssertionError):
    pass


def check_exact(sd, v, types, stats=None):
    """The conditions of `exactness` for several operand types in one pass over the layers: the unfolded forward serves
    fp32 and bf16 and layers 0..7 of fp16, the folded layers 8..10 are run on the same h8.  Returns (float64 outputs,
    {T: the first violation}): a type without an entry meets the conditions.  A violation that does not depend on the type
    (a value that is no multiple of the quantum, a dot product that may pass 2^24 quanta) raises NotExact."""
    v = np.asarray(v, dtype=np.float64)
    why = {}

    def visit_for(Ts, folded=False):
        def visit(L, a, W, b, y):
            used = np.abs(W).sum(0) != 0                                  # input columns that meet a nonzero weight
            n = a[:, used] / QUANTUM
            ni = n.astype(np.int64)
            if (np.rint(b / QUANTUM) * QUANTUM != b).any() or not representable(b, "fp32").all():
                raise NotExact(f"layer {L}: a bias is no fp32 multiple of the quantum")
            if (ni != n).any():
                raise NotExact(f"layer {L}: an input is no multiple of the quantum")
            # the distinct |inputs| of this layer, in quanta: a few hundred small integers
            mags = np.flatnonzero(np.bincount(np.abs(ni).ravel(), minlength=1)) * QUANTUM
            # sum |terms| + |bias| <= max |input| * (largest row sum of |W|) + max |bias|: cheaper than the sum, never smaller
            big = mags.max() * np.abs(W).sum(1).max() + np.abs(b).max()
            if not big < LIMIT:
                raise NotExact(f"layer {L}: a dot product of up to {big / QUANTUM:.0f} quanta")
            for T in Ts:
                if T in why or (T == "fp16" and L >= 8 and not folded):      # fp16 runs layers 8..10 in the folded view, below
                    continue
                if not representable(W, T).all():
                    why[T] = f"{T} layer {L}: a weight is not representable"
                elif not representable(mags, T).all():
                    why[T] = f"{T} layer {L}: an input of magnitude {mags[~representable(mags, T)].max()} is not representable"
            if stats is not None and not folded:
                stats[L] = (float(mags.max() / QUANTUM), float((y > 0).mean()))
        return visit

    out, chain = layer_inputs_from(kernel_layers(sd, "fp32"), v, visit=visit_for(list(types)))
    if "fp16" in types:
        W2, b2 = (sd["layers_2." + k].numpy().astype(np.float64) for k in ("weight", "bias"))
        Wc, bc = (sd["color_fc.0." + k].numpy().astype(np.float64) for k in ("weight", "bias"))
        # the fold itself is an fp32 fma chain in the packer: exact under (c)
        big = max((np.abs(Wc[:, :256]) @ np.abs(W2)).max(), (np.abs(Wc[:, :256]) @ np.abs(b2) + np.abs(bc)).max())
        if not big < LIMIT:
            raise NotExact(f"fold: a partial sum of {big / QUANTUM:.0f} quanta")
        out16, _ = layer_inputs_from(kernel_layers(sd, "fp16"), v, start=8, h=chain[8], visit=visit_for(["fp16"], True))
        if not np.array_equal(out16, out):
            raise NotExact("the folded and the unfolded float64 forward differ")
    if (np.rint(out / QUANTUM) * QUANTUM != out).any() or not representable(out, "fp32").all():
        raise NotExact("an output is not an exact fp32 multiple of the quantum")
    return out, why


def exactness(sd, v, T, stats=None):
    """Asserts, for operand type T on points v [P, 6], (a) every weight as the kernel reads it is representable in T, (b)
    every layer input that meets a nonzero weight is, (c) sum |terms| + |bias| < 2^24 quanta for every dot product, all
    values being multiples of the quantum; returns the float64 outputs [P, 4], which are then what the kernel must return.
    stats (a dict) receives per layer the largest |input| in quanta and the live fraction behind it."""
    out, why = check_exact(sd, v, (T,), stats)
    if why:
        raise NotExact(why[T])
    return out


def emulate(sd, v, T, order=None):
    """The forward as a kernel of operand type T computes it: operands rounded to T (the encoder features and the weights
    once, from float64, with round_to; an fp32 activation by torch's conversion),
    products and sums in fp32.  order None: the bias first, then k ascending in steps of 64; an int seeds a permutation of
    k, summed in steps of 64 with the bias last.  Returns fp32 [P, 4]."""
    def q(a):
        a = np.asarray(a, dtype=np.float64)
        return (a if T == "fp32" else round_to(a, T)).astype(np.float32)

    def q_act(a):                    # an fp32 activation becomes an operand: one rounding, as the kernels' conversions do it
        if T == "fp32":
            return a
        return torch.from_numpy(a).to(torch.bfloat16 if T == "bf16" else torch.float16).float().numpy()

    layers = kernel_layers(sd, T)
    v = np.asarray(v, dtype=np.float64)
    folded = T == "fp16"
    px, pd = q(encode(v[:, :3], LP)), q(encode(v[:, 3:], LD))
    h, sigma = None, None
    for L in range(11):
        a = px if L == 0 else np.concatenate([h, px], 1) if L == 5 else np.concatenate([h, pd], 1) if L == 9 else h
        a = px if L == 0 else q_act(a)
        W, b = q(layers[L][0]), layers[L][1].astype(np.float32)
        K = W.shape[1]
        ks = np.arange(K) if order is None else np.random.Generator(np.random.PCG64(1000 * order + L)).permutation(K)
        acc = np.zeros((len(v), W.shape[0]), np.float32) + (b if order is None else np.float32(0))
        for k0 in range(0, K, 64):
            idx = ks[k0:k0 + 64]
            acc = acc + a[:, idx] @ W[:, idx].T
        y = acc if order is None else acc + b
        if L == 8:
            sigma = y[:, -1:]
            h = h if folded else y[:, :256]
        elif L == 10:
            return np.concatenate([y, sigma], 1)
        else:
            h = np.maximum(y, np.float32(0))


# ---- probe sets -------------------------------------------------------------------------------------------------------------
class ProbeSet:
    def __init__(self, index, name, L, sd, zero=None, part=(1, 0), types=TYPES, out=None):
        self.index, self.name, self.L, self.sd, self.zero, self.part, self.types = index, name, L, sd, zero, part, tuple(types)
        self.half = None                  # layer-8 family: the half of h9 that color_fc.0 selects
        self.out = out                    # float64 outputs [U, 4] on universe(zero): what every kernel must return

    def __repr__(self):
        return f"<set {self.index} {self.name} for {'/'.join(self.types)}>"


def _pm1(rng, shape):
    return rng.integers(0, 2, shape) * 2.0 - 1.0


@functools.lru_cache(maxsize=None)
def _slot_order(L):
    return np.random.Generator(np.random.PCG64(300 + L)).permutation(256 if L != 9 else 128)


def _sparse_bias(L, fam):
    return ((_slot_order(L) + fam) % BIAS_EVERY == 0).astype(np.float64)


def make_state_dict(s, L=None, seed=0, shift=0, part=(1, 0), zero=None, sel=None, fam=None):
    """State dict of set number s (module docstring).  L: the dense layer (None for an encoder set); part = (S, p): the
    p-th of S supports of the dense matrix; shift: the dense layer's biases are -shift + {-1, 0, 1}; zero = c: dense +-1
    on the trig columns of coordinate c (encoder set); sel: the half of h9 that color_fc.0 selects (default fam % 2);
    fam: the number of the set's family (default s), which places the identity layers' biases: every operand type sees every
    family, whatever S, and so every bias slot.
    A dense row carries as many +1 as -1 on its support (one more of either where the support is odd): the common part of
    its inputs -- the biases that the identity layers have added up -- cancels, so that its outputs stay small enough for
    bf16."""
    rng = np.random.Generator(np.random.PCG64([s, seed, 7]))
    fam = s if fam is None else fam
    sel = fam % 2 if sel is None else sel
    sd = {k: np.zeros(shape) for k, shape in PARAM_SPECS}
    S, p = part
    part_rng = np.random.Generator(np.random.PCG64([s - p, seed, 11]))      # the same partition for the S sets of a family

    def dense(rows, cols):
        support = part_rng.integers(0, S, (rows, cols)) == p
        order = np.argsort(rng.random((rows, cols)) + ~support, axis=1)     # per row: its support in random order, first
        signs = np.empty((rows, cols))
        np.put_along_axis(signs, order, np.where(np.arange(cols) % 2 == 0, 1.0, -1.0)[None, :] * _pm1(rng, (rows, 1)), axis=1)
        return signs * support

    for l in range(11):
        W, b = sd[LAYER_KEY[l] + ".weight"], sd[LAYER_KEY[l] + ".bias"]
        rows, K = W.shape
        under = l == L
        if l == 0 and not under:
            w = _pm1(rng, (rows, 3)) * (rng.integers(0, 8, (rows, 3)) != 0)
            w[np.abs(w).sum(1) == 0, 0] = 1.0
            bb = -np.abs(w).sum(1) + rng.integers(0, 2, rows)        # live somewhere in the cube, dead at most points
            for j in range(1, rows):                                 # neighbouring units differ at some point: a weight moved to
                if (w[j] == w[j - 1]).all() and bb[j] == bb[j - 1]:  # the next k, or an input read twice, changes a sum
                    w[j] = -w[j]
            W[:, :3] = w
            b[:] = bb
        elif l == 0:
            W[:, :3] = _pm1(rng, (rows, 3)) * (part_rng.integers(0, S, (rows, 3)) == p)
            b[:] = -shift + rng.integers(-1, 2, rows)
        elif l == 10:
            W[:] = _pm1(rng, W.shape)
            b[:] = rng.integers(-2, 3, rows)
        elif under:
            chain = 256 if l in (5, 9) else K
            W[:, :chain] = dense(rows, chain)
            if l in (5, 9):
                W[:, chain:chain + 3] = _pm1(rng, (rows, 3)) * (part_rng.integers(0, S, (rows, 3)) == p)   # raw coordinates
            b[:] = -shift + rng.integers(-1, 2, rows)
        elif l == 9:
            W[np.arange(128), np.arange(128) + 128 * sel] = 1.0
            b[:] = _sparse_bias(l, fam)
        else:
            W[np.arange(256), np.arange(256)] = 1.0                # identity ([I | 0] for the skip layer)
            b[:] = _sparse_bias(l, fam)
    sd[SIGMA_KEY + ".weight"][:] = _pm1(rng, (1, 256))
    sd[SIGMA_KEY + ".bias"][:] = rng.integers(-2, 3, 1)
    if zero is not None:
        sd[LAYER_KEY[0] + ".weight"][:, trig_cols(zero, LP)] = _pm1(rng, (256, 2 * LP))
        sd[LAYER_KEY[5] + ".weight"][:, 256 + trig_cols(zero, LP)] = _pm1(rng, (256, 2 * LP))
        sd[LAYER_KEY[9] + ".weight"][:, 256 + trig_cols(zero, LD)] = _pm1(rng, (128, 2 * LD))
        # cos = 1 adds the sum of a row's cos weights, an even number in [-L, L], to every point: lift the biases by L, so that
        # no unit is dead at every point because of it
        for l, lift in ((0, LP), (5, LP), (9, LD)):
            sd[LAYER_KEY[l] + ".bias"] += lift
    return {k: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))) for k, a in sd.items()}


LIVE = (0.2, 0.8)
LIVE_TARGET = 0.35
_SEEDS = (0, 1, 2)


def _shift_for(sd0, L):
    """The bias shift that leaves about LIVE_TARGET of layer L's outputs positive: sd0 is the set built with shift 0.  Layers
    8 and 10 have no ReLU behind them: no shift."""
    if L in (8, 10):
        return 0
    ys = {}
    layer_inputs_from(kernel_layers(sd0, "fp32"), universe(None).v,
                      visit=lambda l, a, W, b, y: ys.__setitem__(l, y), stop=L)
    return max(0, int(np.floor(np.quantile(ys[L], 1.0 - LIVE_TARGET))))


def _passes(sd, L, zero):
    """(types whose conditions the set meets, {T: violation}, float64 outputs on the universe); no type at all where the
    live fraction behind a layer L < 8 under test is outside LIVE."""
    stats = {}
    out, why = check_exact(sd, universe(zero).v, TYPES, stats)
    if L is not None and L < 8 and not LIVE[0] <= stats[L][1] <= LIVE[1]:
        why = {T: f"live fraction {stats[L][1]:.2f} behind layer {L}" for T in TYPES}
    return tuple(T for T in TYPES if T not in why), why, out


def _family(s0, L, splits, need, sel=None, fam=None):
    """The sets of the family of layer L, numbered from s0, that serve the types `need`: the smallest S of `splits`, then the
    smallest seed, for which every one of the S sets meets the conditions for them.  Returns (sets, the types they serve)."""
    why = None
    for S in splits:
        for seed in _SEEDS:
            sets, serves = [], TYPES
            for p in range(S):
                shift = _shift_for(make_state_dict(s0 + p, L, seed, 0, (S, p), sel=sel, fam=fam), L)
                sd = make_state_dict(s0 + p, L, seed, shift, (S, p), sel=sel, fam=fam)
                ok, why, out = _passes(sd, L, None)
                serves = tuple(T for T in serves if T in ok)
                if not set(need) <= set(serves):
                    break
                name = f"L{L}" + (f" half {sel}" if sel is not None else "") + f" seed {seed} shift {shift}" + (f" part {p}/{S}" if S > 1 else "")
                sets.append(ProbeSet(s0 + p, name, L, sd, None, (S, p), out=out))
                sets[-1].half = sel
            else:
                return sets, serves
    raise NotExact(f"no probe set for layer {L} and {need}: {why}")


@functools.lru_cache(maxsize=None)
def probe_sets():
    """Every probe set, built once: per layer the dense set for fp32 and fp16, which serves bf16 too where it meets bf16's
    conditions; otherwise S = 2 or 4 sets for bf16 alone.  Then the three encoder sets."""
    sets, n = [], 0
    for L in range(11):
        for sel in ((0, 1) if L == 8 else (None,)):
            fam, serves = _family(len(sets), L, (1,), ("fp32", "fp16"), sel, n)
            fam[0].types = serves
            sets += fam
            if "bf16" not in serves:
                fam, _ = _family(len(sets), L, (2, 4), ("bf16",), sel, n)
                for ps in fam:
                    ps.types = ("bf16",)
                sets += fam
            n += 1
    for c in range(3):
        for seed in _SEEDS:
            sd = make_state_dict(len(sets), None, seed, zero=c, fam=n + c)
            ok, why, out = _passes(sd, None, c)
            if ok == TYPES:
                sets.append(ProbeSet(len(sets), f"encoder coordinate {c} seed {seed}", None, sd, c, out=out))
                break
        else:
            raise NotExact(f"no encoder set for coordinate {c}: {why}")
    return tuple(sets)


def sets_for(T):
    return [ps for ps in probe_sets() if T in ps.types]


def split_table():
    """{layer: S} of the bf16 families (1 where the fp32 / fp16 set serves bf16 too)."""
    return {L: max(ps.part[0] for ps in sets_for("bf16") if ps.L == L) for L in range(11)}


# ---- the same construction at another size (the layer-by-layer path, utils/generic_mlp.py) ---------------------------------------
def small_state_dict(Lp, Ld, H, dense, seed=0):
    """State dict of Nerf(Lp, Ld, H) by the rules of make_state_dict, all integers: the layer named `dense` (a state-dict
    prefix) is dense +-1 on its chain and raw-coordinate columns, the other H-wide layers are the identity plus a bias in
    {0, 1}, color_fc.0 selects one half of h9, sigma_fc.0 and color_fc.2 are dense +-1; the trig columns carry no weight."""
    rng = np.random.Generator(np.random.PCG64([seed, Lp, Ld, H]))
    cx, cd = 3 + 6 * Lp, 3 + 6 * Ld
    shapes = {"layers_0.0": (H, cx), "skip_conn_layer.0": (H, H + cx), "sigma_fc.0": (1, H), "layers_2": (H, H),
              "color_fc.0": (H // 2, H + cd), "color_fc.2": (3, H // 2)}
    names = ("layers_0.0", "layers_0.2", "layers_0.4", "layers_0.6", "layers_0.8", "skip_conn_layer.0", "layers_1.0",
             "layers_1.2", "sigma_fc.0", "layers_2", "color_fc.0", "color_fc.2")
    sd = {}
    for name in names:
        rows, K = shapes.get(name, (H, H))
        W, b = np.zeros((rows, K)), np.zeros(rows)
        if name == "layers_0.0":
            W[:, :3] = _pm1(rng, (rows, 3)) * ((rng.integers(0, 8, (rows, 3)) != 0) | (name == dense))
            W[np.abs(W).sum(1) == 0, 0] = 1.0
            b[:] = -np.abs(W).sum(1) + rng.integers(0, 3, rows)
        elif name in ("sigma_fc.0", "color_fc.2"):
            W[:], b[:] = _pm1(rng, W.shape), rng.integers(-2, 3, rows)
        elif name == dense:
            chain = H if name in ("skip_conn_layer.0", "color_fc.0") else K
            W[:, :min(K, chain + 3)] = _pm1(rng, (rows, min(K, chain + 3)))
            b[:] = rng.integers(-3, 2, rows)
        else:
            W[np.arange(rows), np.arange(rows) + (rows if name == "color_fc.0" and seed % 2 else 0)] = 1.0
            b[:] = rng.integers(0, 2, rows)
        sd[name + ".weight"], sd[name + ".bias"] = W, b
    return {k: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))) for k, a in sd.items()}


# ---- planted faults -----------------------------------------------------------------------------------------------------------
def _copy(layers):
    return [[W.copy(), b.copy()] for W, b in layers]


def fault_move(layers, L, r, k, to=1):
    """The weight at (r, k) multiplies the neighbouring input k + to instead of its own."""
    out = _copy(layers)
    W = out[L][0]
    W[r, k + to] += W[r, k]
    W[r, k] = 0.0
    return out


def fault_zero(layers, L, r, k):
    out = _copy(layers)
    out[L][0][r, k] = 0.0
    return out


def fault_drop_column(layers, L, k):
    out = _copy(layers)
    out[L][0][:, k] = 0.0
    return out


def fault_duplicate_column(layers, L, k):
    """Input k is read in place of input k + 1 as well."""
    out = _copy(layers)
    W = out[L][0]
    W[:, k] += W[:, k + 1]
    W[:, k + 1] = 0.0
    return out


def fault_bias_tile(layers, L, t):
    """The 16 biases of row tile t are those of tile t + 1."""
    out = _copy(layers)
    b = out[L][1]
    nxt = b[16 * t + 16:16 * t + 32]
    b[16 * t:16 * t + len(nxt)] = nxt
    return out


def fault_fragment(layers, L, t, q):
    """The 16-row x 32-k fragment (t, q) holds the fragment before it (1 KiB earlier in a 16-bit image): (t, q - 1)."""
    out = _copy(layers)
    W = out[L][0]
    W[16 * t:16 * t + 16, 32 * q:32 * q + 32] = layers[L][0][16 * t:16 * t + 16, 32 * q - 32:32 * q]
    return out


def fault_folded_bias(layers, sd, r, k):
    """Folded view only: the term Wc[r, k] b2[k] is missing from the colour layer's bias."""
    out = _copy(layers)
    out[9][1][r] -= float(sd["color_fc.0.weight"][r, k]) * float(sd["layers_2.bias"][k])
    return out


def fault_swap_trig(layers, L, c, level):
    """The sin and the cos column of (coordinate c, level) change places in layer L's weight (0, 5: position; 9: direction)."""
    out = _copy(layers)
    W = out[L][0]
    j = (0 if L == 0 else 256) + trig_cols(c, LD if L == 9 else LP)[2 * level]
    W[:, [j, j + 1]] = W[:, [j + 1, j]]
    return out


class FaultBench:
    """Runs planted faults of one set in one kernel view against the set's float64 outputs; the layers before the faulty one
    are not run again."""

    def __init__(self, ps, T):
        self.ps, self.T = ps, T
        self.layers = kernel_layers(ps.sd, T)
        self.v = universe(ps.zero).v
        self.out, self.chain = layer_inputs_from(self.layers, self.v)

    def detected(self, faulty, L):
        got, _ = layer_inputs_from(faulty, self.v, start=L, h=self.chain[L], sigma=self.out[:, 3:])
        return not np.array_equal(got, self.out)
