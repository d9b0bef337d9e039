"""Host model of the bf16 input-gradient stage (csrc/input_grad.hip input_grad_kernel and rays_reduce_kernel), after
tests/train_chain_model.py: the stage is compared element by element with the float64 evaluation of ITS OWN STORED OPERANDS,
under a bound counted from the roundings in the source.  Written from csrc/input_grad.hip and include/nerf_amd.h, never from
what a GPU showed.  Tests: tests/test_input_grad_stage_cpu.py, tests/test_gpu_input_grad_stage.py; DESIGN.md section 8.

Stored operands
    dY0, dY5 [P, 256], dY9 [P, 128]   layers 0, 5, 9 of the point-blocked bf16 buffer nerf_amd_mlp_backward wrote
                                       (train_chain_model.decode_bf16_layers / encode_bf16_layers)
    Wx[c][k], c < 63, k < 512         bf16(layers_0.0.weight[k][c]) for k < 256, bf16(skip_conn_layer.0.weight[k-256][256+c])
                                       behind it: the K = 512 product reads dY0 | dY5
    Wd[c][k], c < 27, k < 128         bf16(color_fc.0.weight[k][256+c])
    the point, fp32                   pts[p] in points mode; the fp32 oracle.query_points(rays, ts) in rays mode (the kernel
                                       recomputes it "exactly as the forward formed it": the tests hold it to that, bit for bit)
Rounding to bf16 is to nearest even (train_chain_model.round_bf16).

Value, in float64
    G[c] = sum_k W[c][k] dY[p][k],   A[c] = sum_k |W[c][k] dY[p][k]|
    J_c  = 1 (raw column), 2^l cos(2^l x) (sin column of level l), -2^l sin(2^l x) (cos column)
    want[p][j] = sum over the columns c of coordinate j of J_c G_c         columns: [x, y, z, g(x), g(y), g(z)],
                                                                           g = [sin l0, cos l0, sin l1, ...]

Bound per element, u = 2^-24, K = 512 (position outputs) or 128 (direction outputs):
    sum_c |J_c| K u A_c                                   the fp32 MFMA sum of K products
  + sum_{c not raw} 2^l (|G_c| + K u A_c)(ENC_ATOL + 2u)  ocml sinf / cosf on the exactly scaled argument (ENC_ATOL: the bound
                                                          the fp32 encoder is held to), the rounding of the trig value's
                                                          product with G_c and of G_c itself
  + T u sum_c |J_c| (|G_c| + K u A_c)                     the additions into one output: 21 (9) terms over the four lane
                                                          groups, the two butterfly steps; T = 24 (12)
On integer operands with every A_c < 2^24 (asserted) the products and every partial sum of G are exact in fp32 whatever the
order, so the K u A_c terms are zero and dropped.  Where every term but one is an exact zero (one-hot operands) the additions
round nothing either: T = 0.

The acceptance rule is |got - want| <= bound for every element (``ratio``: |got - want| / bound, 0 / 0 = 0, anything
non-finite or x / 0 = inf); the worst ratio is printed by the tests as an output, not a tolerance.

rays_reduce (samples -> rays), float64:  d_o = sum_n dx_n,  d_d = sum_n t_n dx_n + (g - dh (dh . g)) / |d|,  g = sum_n du_n,
dh = d / |d|.  Bound, with gamma(n) = n u / (1 - n u): each sum of N terms costs gamma(N) of its absolute mass; behind them,
counted from rays_reduce_kernel: the norm (one product, two fmas: 3 roundings of the sum of squares, halved by the root, plus
the root's own: 2.5), a division (dh_k: 3.5), the dot product (three more on each term: 6.5), its product with dh_k (11), the
bracket (12), the division by |d| (15.5) and the last addition (16.5): gamma(17) on (|g_k| + |dh_k| sum_m |dh_m g_m|) / |d|
and gamma(N + 1) on the mass of sum_n t_n dx_n.  A contracted fma only removes roundings.
"""
import numpy as np

import train_chain_model as C
from encoder_probe_model import ENC_ATOL

U = 2.0 ** -24
LP, LD = 10, 4
NX, ND = 3 + 6 * LP, 3 + 6 * LD              # 63, 27
KX, KD = 512, 128
T_POS, T_DIR = 24, 12
GUARD = 64                                   # floats behind dv [P, 6] that must stay untouched
POISON_BITS = 0x40E0                         # bf16 7.0: features 128..255 of layer 9, no operand of anything
DV_FILL_BITS = 0x7FC5A5A5                    # the quiet NaN dv and its guard hold before the launch
ENTRIES = NX + NX + ND                       # 153 (slab, column) pairs: W0, the skip slice, the C0 slice


def columns(L):
    """(coordinate, level, trig) per column of an encoder output [v0, v1, v2, g(v0), g(v1), g(v2)]; level -1: raw."""
    coord = np.concatenate([np.arange(3), np.repeat(np.arange(3), 2 * L)])
    level = np.concatenate([np.full(3, -1), np.tile(np.repeat(np.arange(L), 2), 3)])
    trig = np.concatenate([np.zeros(3, dtype=np.int64), np.tile(np.tile([0, 1], L), 3)])
    return coord, level, trig


# ---- operands ------------------------------------------------------------------------------------------------------------
def _mat(params, name):
    off, shape = C.OFFSETS[name]
    return np.asarray(params, dtype=np.float32)[off:off + int(np.prod(shape))].reshape(shape)


def stored_weights(params):
    """(Wx [63, 512], Wd [27, 128]) float64: the bf16 operands of the two products, from the flat fp32 parameter vector."""
    w0 = _mat(params, "layers_0.0.weight")
    w5 = _mat(params, "skip_conn_layer.0.weight")[:, 256:256 + NX]
    c0 = _mat(params, "color_fc.0.weight")[:, 256:256 + ND]
    wx = np.ascontiguousarray(np.concatenate([w0, w5], axis=0).T)
    wd = np.ascontiguousarray(c0.T)
    return C.round_bf16(wx).astype(np.float64), C.round_bf16(wd).astype(np.float64)


def stored_dys(host, P):
    """(dY0, dY5 [P, 256], dY9 [P, 128]) float64 from the bf16 buffer."""
    dY = C.decode_bf16_layers(host, P)
    return dY[0].astype(np.float64), dY[5].astype(np.float64), dY[9][:, :128].astype(np.float64)


def flat_params(sd):
    """fp32 [595844] numpy vector of a state dict, in state_dict order."""
    return np.concatenate([np.asarray(sd[k], dtype=np.float32).reshape(-1) for k, _ in C.PARAM_SPECS])


# ---- the stage -----------------------------------------------------------------------------------------------------------
def _half(dY, W, x, L, K, T, integer):
    G, A = dY @ W.T, np.abs(dY) @ np.abs(W).T
    coord, level, trig = columns(L)
    scale = np.where(level >= 0, 2.0 ** np.maximum(level, 0), 0.0)
    a = x[:, coord] * np.where(level >= 0, scale, 1.0)               # exact: a power of two times an fp32 value
    J = np.where(level < 0, 1.0, np.where(trig == 0, scale * np.cos(a), -scale * np.sin(a)))
    if integer:
        assert np.array_equal(G, np.round(G)) and (A < 2.0 ** 24).all()
        ku = 0.0
    else:
        ku = K * U * A
    Gm = np.abs(G) + ku
    e = np.abs(J) * ku + scale * Gm * (ENC_ATOL + 2 * U) + T * U * np.abs(J) * Gm
    onehot = (coord[:, None] == np.arange(3)[None, :]).astype(np.float64)
    return (J * G) @ onehot, e @ onehot


def stage(dY0, dY5, dY9, Wx, Wd, pts, integer=False, t_pos=T_POS, t_dir=T_DIR):
    """(want [P, 6], bound [P, 6]) of dv from the stored operands (module docstring).  pts [P, 6] fp32."""
    f8 = lambda a_: np.asarray(a_, dtype=np.float64)
    assert np.asarray(pts).dtype == np.float32
    v = f8(pts)
    wx, bx = _half(np.concatenate([f8(dY0), f8(dY5)], axis=1), f8(Wx), v[:, :3], LP, KX, t_pos, integer)
    wd, bd = _half(f8(dY9), f8(Wd), v[:, 3:], LD, KD, t_dir, integer)
    return np.concatenate([wx, wd], axis=1), np.concatenate([bx, bd], axis=1)


def exact_at_origin(dY0, dY5, dY9, Wx, Wd):
    """dv at pts = 0 (cosf(0) = 1, sinf(0) = 0 exactly): G_raw + sum_l 2^l G_sin[l] per coordinate, and the largest sum of
    absolute terms (the result is exact in fp32, in any order, while that stays below 2^24 units of the operands' grid)."""
    f8 = lambda a_: np.asarray(a_, dtype=np.float64)
    out, mass = [], 0.0
    for dY, W, L in ((np.concatenate([f8(dY0), f8(dY5)], axis=1), f8(Wx), LP), (f8(dY9), f8(Wd), LD)):
        G, A = dY @ W.T, np.abs(dY) @ np.abs(W).T
        coord, level, trig = columns(L)
        w = np.where(level < 0, 1.0, np.where(trig == 0, 2.0 ** np.maximum(level, 0), 0.0))
        onehot = (coord[:, None] == np.arange(3)[None, :]).astype(np.float64)
        out.append((G * w) @ onehot)
        mass = max(mass, float(((A * w) @ onehot).max()))
    return np.concatenate(out, axis=1), mass


def ratio(got, want, bound):
    """|got - want| / bound per element; 0 where both are 0, inf where got is not finite or the bound is 0 and got differs."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), r, np.inf)


def gamma_n(n):
    return n * U / (1.0 - n * U)


def rays_reduce(rays, ts, d_q):
    """(want [B, 6], bound [B, 6]) of d_rays from rays [B, 6], ts [B, N] (fp32) and the stored d_q [B*N, 6] (fp32)."""
    rays, ts, d_q = (np.asarray(a_) for a_ in (rays, ts, d_q))
    assert rays.dtype == ts.dtype == d_q.dtype == np.float32
    B, N = ts.shape
    q = d_q.astype(np.float64).reshape(B, N, 6)
    t = ts.astype(np.float64)[:, :, None]
    d = rays[:, 3:].astype(np.float64)
    nrm = np.sqrt((d * d).sum(1, keepdims=True))
    dh = d / nrm
    dx, du = q[:, :, :3], q[:, :, 3:]
    d_o, m_o = dx.sum(1), np.abs(dx).sum(1)
    s_d, m_d = (t * dx).sum(1), np.abs(t * dx).sum(1)
    g, m_g = du.sum(1), np.abs(du).sum(1)
    through = lambda e: (e + np.abs(dh) * (np.abs(dh) * e).sum(1, keepdims=True)) / nrm      # a perturbation of g, at the output
    want = np.concatenate([d_o, s_d + (g - dh * (dh * g).sum(1, keepdims=True)) / nrm], axis=1)
    M = (np.abs(g) + np.abs(dh) * np.abs(dh * g).sum(1, keepdims=True)) / nrm
    b_d = gamma_n(N + 1) * m_d + gamma_n(17) * M + (1 + gamma_n(17)) * gamma_n(N) * through(m_g)
    return want, np.concatenate([gamma_n(N) * m_o, b_d], axis=1)


# ---- crafted buffers ------------------------------------------------------------------------------------------------------
def bf16_bits(v):
    """uint16 patterns of float32 values that are exact in bf16 (non-finite ones included)."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    assert not (b & 0xFFFF).any()
    return (b >> 16).astype(np.uint16)


def layer_bytes(P):
    return C.act_tiles(P) * C.ACT_BLOCK_BYTES


def craft_layer(v, P):
    """One layer of the point-blocked buffer, uint8 [layer_bytes(P)], from v [P, 256] or [P, 128] (layer 9: features
    128..255 then hold the finite poison 7.0); granules of points >= P hold 0xFFFF."""
    nt = C.act_tiles(P)
    bits = np.full((nt * 256, 256), 0xFFFF, dtype=np.uint16)
    bits[:P, :v.shape[1]] = bf16_bits(v)
    if v.shape[1] == 128:
        bits[:P, 128:] = POISON_BITS
    return np.ascontiguousarray(bits.reshape(nt, 256, 32, 8).transpose(0, 2, 1, 3)).reshape(-1).view(np.uint8)


def craft_layers(dY0, dY5, dY9, P):
    """{layer: bytes} of the three layers the kernel reads; each goes to byte offset layer * layer_bytes(P)."""
    assert dY0.shape == dY5.shape == (P, 256) and dY9.shape == (P, 128)
    return {0: craft_layer(dY0, P), 5: craft_layer(dY5, P), 9: craft_layer(dY9, P)}


def craft_dys(dY0, dY5, dY9, P):
    """The whole bf16 part of the buffer on the host: the seven layers the kernel does not read are 0xFFFF (bf16 NaN)."""
    buf = np.full(C.acts_bf16_bytes(P), 0xFF, dtype=np.uint8)
    n = layer_bytes(P)
    for L, b in craft_layers(dY0, dY5, dY9, P).items():
        buf[L * n:(L + 1) * n] = b
    return buf


def craft_params(W0, W5s, C0s):
    """The flat fp32 parameter vector, NaN but for the three slices the kernel reads: W0 [256, 63] = layers_0.0.weight,
    W5s [256, 63] = columns 256..318 of skip_conn_layer.0.weight, C0s [128, 27] = columns 256..282 of color_fc.0.weight."""
    p = np.full(C.PARAM_COUNT, np.nan, dtype=np.float32)
    assert W0.shape == W5s.shape == (256, NX) and C0s.shape == (128, ND)
    _mat(p, "layers_0.0.weight")[:] = W0
    _mat(p, "skip_conn_layer.0.weight")[:, 256:256 + NX] = W5s
    _mat(p, "color_fc.0.weight")[:, 256:256 + ND] = C0s
    return p


# ---- the committed cases (shared by the CPU and the GPU tests) -----------------------------------------------------------
def general_points(P, seed):
    """[P, 6] fp32: positions uniform in [-4.5, 4.5), direction columns in [-1, 1) -- the range of the golden vectors
    (synthetic.points_in_scene) on which tests/test_gpu_parity.py holds the fp32 encoder (the same sinf / cosf on the same
    exactly scaled argument) to ENC_ATOL."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.concatenate([rng.uniform(-4.5, 4.5, size=(P, 3)), rng.uniform(-1.0, 1.0, size=(P, 3))], axis=1).astype(np.float32)


def _case(P, dY0, dY5, dY9, W0, W5s, C0s, pts, **kw):
    f4 = lambda a_: np.ascontiguousarray(a_, dtype=np.float32)
    return dict(P=P, dY0=f4(dY0), dY5=f4(dY5), dY9=f4(dY9), params=craft_params(f4(W0), f4(W5s), f4(C0s)), pts=f4(pts), **kw)


def case_integers(P, seed, origin):
    """Integer dY and integer weights in [-2, 2]; points at the origin (cases a) or general (case d)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    r = lambda *s: rng.integers(-2, 3, size=s, dtype=np.int8)
    pts = np.zeros((P, 6), dtype=np.float32) if origin else general_points(P, seed + 1)
    return _case(P, r(P, 256), r(P, 256), r(P, 128), r(256, NX), r(256, NX), r(128, ND), pts, integer=True)


ROUNDING_WEIGHTS = np.array([1 + 2.0 ** -8,                 # a tie: to the even neighbour, 1
                             1 + 2.0 ** -8 + 2.0 ** -20,    # above the tie: 1 + 2^-7
                             1 + 2.0 ** -7 + 2.0 ** -8],    # a tie whose even neighbour is the upper one: 1 + 2^-6
                            dtype=np.float32)
ROUNDED_WEIGHTS = np.array([1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -6])


def case_rounding(P, seed):
    """Case b: points at the origin, integer dY in [-2, 2], weights +-ROUNDING_WEIGHTS.  Each column of a slab carries 16
    nonzero weights (the rest are zero), which keeps the sum of the absolute terms of every output below 2^17: the operands
    sit on a grid of 2^-7, so every partial sum has at most 24 significant bits and the fp32 result is exact in any order
    (exact_at_origin returns that sum; the tests assert it)."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def slab(K, ncol):
        w = np.zeros((K, ncol), dtype=np.float32)
        for c in range(ncol):
            k = rng.choice(K, size=16, replace=False)
            w[k, c] = ROUNDING_WEIGHTS[rng.integers(0, 3, size=16)] * rng.choice([-1.0, 1.0], size=16).astype(np.float32)
        return w

    r = lambda *s: rng.integers(-2, 3, size=s, dtype=np.int8)
    return _case(P, r(P, 256), r(P, 256), r(P, 128), slab(256, NX), slab(256, NX), slab(128, ND),
                 np.zeros((P, 6), dtype=np.float32), integer=False)


ONEHOT_VALUES = (1.0, -1.0, 2.0, -2.0)


def case_onehot(P, seed=0):
    """Case c: identity slabs (W[k][c] = delta(k, c)) in all three slices; point p carries ONE nonzero dY entry, entry
    p % 153 of (dY0 columns 0..62 | dY5 columns 0..62 | dY9 columns 0..26), with the value ONEHOT_VALUES[(p // 153) % 4]: its
    dv is one Jacobian term in one output and exact zeros in the other five."""
    eye = lambda K, n: np.eye(K, n, dtype=np.float32)
    dY0, dY5, dY9 = np.zeros((P, 256), np.float32), np.zeros((P, 256), np.float32), np.zeros((P, 128), np.float32)
    p = np.arange(P)
    e = p % ENTRIES
    val = np.asarray(ONEHOT_VALUES, dtype=np.float32)[(p // ENTRIES) % 4]
    for dY, lo, n in ((dY0, 0, NX), (dY5, NX, NX), (dY9, 2 * NX, ND)):
        sel = (e >= lo) & (e < lo + n)
        dY[p[sel], e[sel] - lo] = val[sel]
    return _case(P, dY0, dY5, dY9, eye(256, NX), eye(256, NX), eye(128, ND), general_points(P, 77 + seed), integer=True,
                 entry=e, value=val)


def expect(case):
    """(want, bound) of a committed case: the exact cases have bound 0 everywhere."""
    Wx, Wd = stored_weights(case["params"])
    args = (case["dY0"], case["dY5"], case["dY9"], Wx, Wd)
    if not case["pts"].any():
        want, mass = exact_at_origin(*args)
        grid = 1.0 if case["integer"] else 2.0 ** -7
        assert mass < 2.0 ** 24 * grid, mass
        return want, np.zeros_like(want)
    if "entry" in case:
        return stage(*args, case["pts"], integer=True, t_pos=0, t_dir=0)
    return stage(*args, case["pts"], integer=case["integer"])


def crafted_rays(B, N, seed):
    """rays [B, 6] and sorted ts [B, N] (fp32) whose query points stay inside [-4.5, 4.5]: origins in [-2, 2], directions of
    length 0.1 .. 0.4 (NOT unit: the normalisation matters), ts in [2, 6]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = rng.standard_normal((B, 3))
    d *= rng.uniform(0.1, 0.4, (B, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    o = rng.uniform(-2.0, 2.0, (B, 3))
    ts = np.sort(rng.uniform(2.0, 6.0, (B, N)), axis=1)
    return np.ascontiguousarray(np.concatenate([o, d], axis=1).astype(np.float32)), np.ascontiguousarray(ts.astype(np.float32))
