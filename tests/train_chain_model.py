"""Host model of the bf16 training step, stage by stage (test infrastructure, after tests/error_model.py and
tests/input_grad_model.py).

Every stage of the step -- the saving forward (csrc/mlp_bf16_16.hip), the dX chain (csrc/mlp_bwd_16.hip), the 14 products
and the bias sums (csrc/dw_gemm.hip) -- writes its result to HBM in a documented layout (csrc/nerf_layout.h).  So each
stage is checked against a float64 evaluation of ITS OWN STORED INPUTS, and bf16 noise does not accumulate from stage to
stage: what is left is the fp32 accumulation of one dot product and, where the stage stores bf16, one rounding.

The acceptance rule (``stage_ratio``), with no fitted constant.  For a stage that sums K products in fp32:

    |got - y| <= delta,                       delta = (K + 2) * 2^-23 * mass + 2^-126

``mass`` is the sum of the absolute values of the terms of y (bias included): the a-priori bound of a length-K fp32 sum in
any order; 2^-23 instead of 2^-24 so that it holds whether the MFMA accumulator rounds to nearest or truncates; 2^-126 (the
smallest normal number of fp32 and of bf16) because the hardware may flush what lies below it.  For a stage that then stores
bf16:

    |got - y| <= delta + 1/2 ulp_bf16(|y| + delta),      ulp_bf16(t) = 2^(floor(log2 t) - 7)

Where a ReLU mask bit is 0 the stored dY must be exactly 0; where y < -delta a stored ReLU output must be exactly 0; stored
ReLU outputs are never negative.  A violated exactness rule counts as ratio = inf.  For the products over the points the
number of summed terms is P plus the split-K partials (at most the workgroup count, 256): delta = (P + 258) * 2^-23 * mass.

Encoder columns: layers 0, 5 (skip) and 9 (colour) also consume encoder features that the fused forward forms in registers
while the rows the products read come from nerf_amd_sample_encode_bf16; the two encoders differ by ~1e-6 before rounding, so
a stored row can sit one bf16 step from what the forward used.  ``delta_enc = sum_k |w16_k| (ulp_bf16(x_k) + 2^-19)`` over
the encoder columns is added to delta for those layers (zero for a weight set whose encoder columns are zero:
``zero_encoder_columns``).  The in-register encoder itself is pinned elsewhere, feature by feature against float64:
tests/test_gpu_encoder_probe.py (probe weight sets that turn single encoder columns into outputs).

``emulate_chain`` is a CPU emulation of the whole chain (bf16 round-to-nearest-even storage, fp32 sums in one of two orders)
that produces the same buffers as the kernels; tests/test_train_chain_model_cpu.py runs it through the rule, unharmed and
with planted faults.
"""
import numpy as np
import torch

from nerf_simple_amd.utils.synthetic import PARAM_SPECS, PARAM_COUNT

NUM_ACT = 10
ACT_TILE_PTS = 256
ACT_BLOCK_BYTES = 256 * 512
U23 = 2.0 ** -23
FLUSH = 2.0 ** -126
SPLIT_K_PARTIALS = 256
# internal layer L of csrc/nerf_layout.h -> state-dict name of the layer that produces X[L] / owns dY[L]
LAYER_NAMES = ("layers_0.0", "layers_0.2", "layers_0.4", "layers_0.6", "layers_0.8", "skip_conn_layer.0", "layers_1.0",
               "layers_1.2", "layers_2", "color_fc.0")
RELU = (1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
OFFSETS = {}
_o = 0
for _k, _s in PARAM_SPECS:
    OFFSETS[_k] = (_o, _s)
    _o += int(np.prod(_s))
assert _o == PARAM_COUNT == 595844


def act_width(L):
    return 128 if L == 9 else 256


def act_tiles(P):
    return (P + ACT_TILE_PTS - 1) // ACT_TILE_PTS


def acts_bf16_bytes(P):
    return NUM_ACT * act_tiles(P) * ACT_BLOCK_BYTES


# ---- layout ------------------------------------------------------------------------------------------------------------
def bf16_to_f32(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(x):
    """uint16 bit patterns of x rounded to bf16, round-to-nearest-even (torch's .bfloat16(); the kernels' (__bf16) cast)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


def round_bf16(x):
    """x (float32 array) rounded to bf16 and back."""
    return bf16_to_f32(f32_to_bf16_bits(x))


def decode_bf16_layers(host, P):
    """[10][P, 256] float32 from the point-blocked bf16 buffer (nerf_layout.h act_elem_offset)."""
    nt = act_tiles(P)
    out = []
    for L in range(NUM_ACT):
        blk = host[L * nt * ACT_BLOCK_BYTES:(L + 1) * nt * ACT_BLOCK_BYTES].view(np.uint16).reshape(nt, 32, 256, 8)
        out.append(bf16_to_f32(blk.transpose(0, 2, 1, 3).reshape(nt * 256, 256)[:P]))
    return out


def encode_bf16_layers(layers, P, fill=0xFFFF):
    """The inverse: [10][P, 256] values (exact in bf16) -> the bf16 part of the buffer as uint8 [acts_bf16_bytes(P)].  Granules
    of points >= P in the last tile hold the bit pattern ``fill`` (0xFFFF: a bf16 NaN)."""
    nt = act_tiles(P)
    out = np.empty((NUM_ACT, nt * 256, 256), dtype=np.uint16)
    out[:, P:, :] = fill
    for L in range(NUM_ACT):
        out[L, :P] = f32_to_bf16_bits(layers[L])
    blocked = out.reshape(NUM_ACT, nt, 256, 32, 8).transpose(0, 1, 3, 2, 4)        # [L][tile][chunk][point][8]
    return np.ascontiguousarray(blocked).reshape(-1).view(np.uint8)


def decode_masks(host, P):
    """[10][P, 256] bool from the ReLU mask dwords behind the bf16 activations (nerf_layout.h: per (layer, tile of 256
    points) 4 dwords x 512 threads; thread (wave, lane), column block cb, fragment Q: dword cb*2 + (Q>>2), bit (Q&3)*4 + j
    + 16 e <-> feature 32Q + 16(j>>1) + 4(lane>>4) + 2(j&1) + e of point wave*32 + cb*16 + (lane&15)).  Layer 8 has no ReLU
    and layer 9 is 128 wide: what decodes there beyond is whatever the buffer held."""
    nt = act_tiles(P)
    region = acts_bf16_bytes(P)
    m = host[region:region + NUM_ACT * nt * 8192].view(np.uint32).reshape(NUM_ACT, nt, 4, 512)
    bits = ((m[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)     # [L, tile, dword, tid, bit]
    dword, tid, bit = np.meshgrid(np.arange(4), np.arange(512), np.arange(32), indexing="ij")
    wave, lane = tid >> 6, tid & 63
    cb, e, r = dword >> 1, bit >> 4, bit & 15
    Q, j = (dword & 1) * 4 + (r >> 2), r & 3
    pt = wave * 32 + cb * 16 + (lane & 15)
    feat = 32 * Q + 16 * (j >> 1) + 4 * (lane >> 4) + 2 * (j & 1) + e
    out = np.zeros((NUM_ACT, nt, 256, 256), dtype=bool)
    out[:, :, pt, feat] = bits
    return [out[L].reshape(nt * 256, 256)[:P] for L in range(NUM_ACT)]


def decode_d_raw_rows(scratch, P):
    """[P, 32] float32: the packed d_raw rows at the head of the dW scratch (bf16; columns 0..2 d_rgb, 3 d_sigma, rest 0)."""
    return bf16_to_f32(scratch[:P * 64].view(np.uint16).reshape(P, 32))


# ---- weights -----------------------------------------------------------------------------------------------------------
def w16(sd):
    """float64 arrays: weights rounded to bf16 (round-to-nearest-even, as the packers round them), biases as they are."""
    out = {}
    for k, v in sd.items():
        v = torch.as_tensor(v).float()
        out[k] = (v.bfloat16().float() if k.endswith("weight") else v).double().numpy()
    return out


def zero_encoder_columns(sd):
    """``sd`` with the encoder columns of the skip layer and of the colour layer zeroed: layers 1..9 are then exact in their
    stored operands."""
    out = {k: torch.as_tensor(v).clone() for k, v in sd.items()}
    out["skip_conn_layer.0.weight"][:, 256:] = 0
    out["color_fc.0.weight"][:, 256:] = 0
    return out


# ---- the rule ----------------------------------------------------------------------------------------------------------
def ulp_bf16(t):
    t = np.maximum(np.abs(t), FLUSH)
    return 2.0 ** (np.floor(np.log2(t)) - 7)


def stage_ratio(got, y, mass, K, store_bf16, relu=False, mask=None, extra_delta=0.0):
    """Worst |got - y| / bound over the stage's elements (module docstring); inf if an exactness rule is broken."""
    got = np.asarray(got, dtype=np.float64)
    delta = (K + 2) * U23 * mass + FLUSH + extra_delta
    want = y
    if mask is not None:
        want = np.where(mask, y, 0.0)
        if (got[~mask] != 0).any():
            return float("inf")
    if relu:
        want = np.maximum(want, 0.0)
        if (got < 0).any() or (got[y < -delta] != 0).any():
            return float("inf")
    if not np.isfinite(got).all():
        return float("inf")
    bound = delta + (0.5 * ulp_bf16(np.abs(want) + delta) if store_bf16 else 0.0)
    return float((np.abs(got - want) / bound).max()) if got.size else 0.0


def _lin(X, W, b=None):
    """(y, mass) of X @ W^T (+ b) in float64."""
    y, mass = X @ W.T, np.abs(X) @ np.abs(W).T
    if b is not None:
        y, mass = y + b, mass + np.abs(b)
    return y, mass


def delta_enc(rows, Wenc):
    """sum_k |w16_k| (ulp_bf16(x_k) + 2^-19) over encoder columns: rows [P, n] stored encoder rows, Wenc [out, n]."""
    return (np.where(rows != 0, ulp_bf16(rows), 0.0) + 2.0 ** -19) @ np.abs(Wenc).T


def forward_stage(L, W, X, posx, posd):
    """(y, mass, K, delta_enc) of the pre-activation of internal layer L (0..9) from the stored operands: X the list of
    decoded activations (float64), posx [P, 63] / posd [P, 27] the stored encoder rows."""
    name = LAYER_NAMES[L]
    Wl, b = W[name + ".weight"], W[name + ".bias"]
    if L == 0:
        y, m = _lin(posx, Wl, b)
        return y, m, 63, delta_enc(posx, Wl)
    src = X[L - 1] if L != 9 else X[8]
    y, m = _lin(src[:, :256], Wl[:, :256], b)
    if L in (5, 9):
        rows = posx if L == 5 else posd
        ye, me = _lin(rows, Wl[:, 256:])
        return y + ye, m + me, Wl.shape[1], delta_enc(rows, Wl[:, 256:])
    return y, m, 256, 0.0


def head_stages(W, X):
    """{'raw.sigma': (y, mass, K), 'raw.rgb': ...}: raw[:, 3] = sigma_fc . X[7] + b, raw[:, :3] = color_fc.2 . X[9] + b."""
    ys, ms = _lin(X[7], W["sigma_fc.0.weight"], W["sigma_fc.0.bias"])
    yc, mc = _lin(X[9][:, :128], W["color_fc.2.weight"], W["color_fc.2.bias"])
    return {"raw.sigma": (ys, ms, 256), "raw.rgb": (yc, mc, 128)}


def dx_stage(L, W, dY, dsr):
    """(y, mass, K) of dY[L] BEFORE its mask, from the stored dY[L + 1] and the bf16 d_raw (dsr [P, >= 4], columns 0..2 d_rgb,
    3 d_sigma), in the order of nerf_layout.h bwd_desc."""
    if L == 9:
        y, m = _lin(dsr[:, :3], W["color_fc.2.weight"].T)
        return y, m, 3
    if L == 8:
        y, m = _lin(dY[9][:, :128], W["color_fc.0.weight"][:, :256].T)
        return y, m, 128
    if L == 7:
        y, m = _lin(dY[8], W["layers_2.weight"].T)
        ys, ms = _lin(dsr[:, 3:4], W["sigma_fc.0.weight"].T)
        return y + ys, m + ms, 257
    y, m = _lin(dY[L + 1], W[LAYER_NAMES[L + 1] + ".weight"][:, :256].T)
    return y, m, 256


def expected_param_grads(X, dY, posx, posd, dsr, d_raw, with_mass=True):
    """(y, mass): the flat 595,844-entry gradient vector in float64 and the mass of every entry -- the 14 products and the
    bias sums of nerf_amd_launch_param_gradients_finish (the table DW_PRODUCTS in csrc/dw_products.h), head biases from the
    fp32 d_raw.  posx [P, >= 63], posd [P, >= 27]: only the true columns enter.  ``with_mass=False`` leaves the mass at zero
    (the exact-integer test needs none)."""
    y, mass = np.zeros(PARAM_COUNT), np.zeros(PARAM_COUNT)

    def put(name, A, B=None):
        off, shape = OFFSETS[name]
        n = int(np.prod(shape))
        y[off:off + n] = (A.sum(0) if B is None else A.T @ B).reshape(-1)
        if with_mass:
            mass[off:off + n] = (np.abs(A).sum(0) if B is None else np.abs(A).T @ np.abs(B)).reshape(-1)

    posx, posd = posx[:, :63], posd[:, :27]
    put("layers_0.0.weight", dY[0], posx)
    put("layers_0.0.bias", dY[0])
    for L in (1, 2, 3, 4, 6, 7, 8):
        put(LAYER_NAMES[L] + ".weight", dY[L], X[L - 1])
        put(LAYER_NAMES[L] + ".bias", dY[L])
    put("skip_conn_layer.0.weight", dY[5], np.concatenate([X[4], posx], axis=1))
    put("skip_conn_layer.0.bias", dY[5])
    put("sigma_fc.0.weight", dsr[:, 3:4], X[7])
    put("sigma_fc.0.bias", d_raw[:, 3:4])
    put("color_fc.0.weight", dY[9][:, :128], np.concatenate([X[8], posd], axis=1))
    put("color_fc.0.bias", dY[9][:, :128])
    put("color_fc.2.weight", dsr[:, :3], X[9][:, :128])
    put("color_fc.2.bias", d_raw[:, :3])
    return y, mass


def check_chain(bufs, sd, enc_slack=True):
    """Every stage of one training step against the float64 evaluation of its stored operands.  ``bufs``: X, dY ([10][P, 256]),
    masks ([10][P, 256] bool), raw, d_raw ([P, 4] fp32), dsr ([P, 32] decoded packed d_raw), posx ([P, 64]), posd ([P, 32]),
    grads (flat fp32).  Returns {stage: worst |got - y| / bound}; the step passes when every value is <= 1."""
    f8 = lambda a: np.asarray(a, dtype=np.float64)
    W = w16(sd)
    X, dY = [f8(a) for a in bufs["X"]], [f8(a) for a in bufs["dY"]]
    masks = bufs["masks"]
    posx64, posd32, d_raw, dsr = f8(bufs["posx"]), f8(bufs["posd"]), f8(bufs["d_raw"]), f8(bufs["dsr"])
    posx, posd = posx64[:, :63], posd32[:, :27]
    P = X[0].shape[0]
    res = {}
    for L in range(NUM_ACT):
        w = act_width(L)
        y, m, K, de = forward_stage(L, W, X, posx, posd)
        res[f"X[{L}]"] = stage_ratio(X[L][:, :w], y, m, K, True, relu=bool(RELU[L]), extra_delta=de if enc_slack else 0.0)
        if RELU[L]:
            res[f"mask[{L}]"] = 0.0 if np.array_equal(masks[L][:, :w], X[L][:, :w] != 0) else float("inf")
    raw = f8(bufs["raw"])
    for k, (y, m, K) in head_stages(W, X).items():
        res[k] = stage_ratio(raw[:, 3:4] if k == "raw.sigma" else raw[:, :3], y, m, K, False)
    exact = np.array_equal(dsr[:, :4], f8(round_bf16(bufs["d_raw"]))) and not dsr[:, 4:].any()
    res["d_raw.pack"] = 0.0 if exact else float("inf")
    for L in range(NUM_ACT - 1, -1, -1):
        w = act_width(L)
        y, m, K = dx_stage(L, W, dY, dsr)
        res[f"dY[{L}]"] = stage_ratio(dY[L][:, :w], y, m, K, True, mask=masks[L][:, :w] if RELU[L] else None)
    y, mass = expected_param_grads(X, dY, posx, posd, dsr, d_raw)
    grads = f8(bufs["grads"])
    assert grads.shape == (PARAM_COUNT,)
    for name, (off, shape) in OFFSETS.items():
        n = int(np.prod(shape))
        tag = ("dW " if name.endswith("weight") else "db ") + name
        res[tag] = stage_ratio(grads[off:off + n], y[off:off + n], mass[off:off + n], P + SPLIT_K_PARTIALS, False)
    return res


def report(res, title=""):
    """One line per group of stages: the worst ratio and where."""
    groups = {}
    for k, v in res.items():
        g = k.split("[")[0].split(" ")[0]
        if g not in groups or v > groups[g][1]:
            groups[g] = (k, v)
    return title + " " + "  ".join(f"{g}: {v:.4f} ({k})" for g, (k, v) in groups.items())


# ---- CPU emulation of the chain ----------------------------------------------------------------------------------------
def _mm(a, bt, order, rng, chunks=None):
    """a [M, K] @ bt [K, N] in fp32: 'plain' = one matmul, 'split' = 32-wide k slabs added in shuffled order.  ``chunks``
    (slab indices, repeats allowed) overrides the set of slabs: the planted split-K faults."""
    K = a.shape[1]
    if order == "plain" and chunks is None:
        return a @ bt
    ns = (K + 31) // 32
    idx = list(range(ns)) if chunks is None else list(chunks)
    if order == "split":
        idx = [idx[i] for i in rng.permutation(len(idx))]
    acc = torch.zeros(a.shape[0], bt.shape[1])
    for s in idx:
        acc = acc + a[:, 32 * s:32 * s + 32] @ bt[32 * s:32 * s + 32]
    return acc


def _store(x, truncate=False):
    if truncate:
        return (x.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32)
    return x.bfloat16().float()


def emulate_chain(sd, posx64, posd32, d_raw, order="plain", seed=0, fault=None):
    """The bf16 training step on the CPU: bf16 round-to-nearest-even storage, fp32 sums (``order``: 'plain' or 'split'), from
    the stored encoder rows posx64 [P, 64] / posd32 [P, 32] (bf16-valued fp32; pad columns are never used) and the fp32 d_raw
    [P, 4].  Returns the buffers ``check_chain`` takes.  ``fault`` plants one defect (tests/test_train_chain_model_cpu.py)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    Wt = {k: (torch.as_tensor(v).float().bfloat16().float() if k.endswith("weight") else torch.as_tensor(v).float())
          for k, v in sd.items()}
    posx, posd = posx64[:, :63], posd32[:, :27]
    P = posx.shape[0]
    X, masks = [], []
    for L in range(NUM_ACT):
        name = LAYER_NAMES[L]
        Wl, b = Wt[name + ".weight"], Wt[name + ".bias"]
        if L == 0:
            acc = _mm(posx, Wl.T.contiguous(), order, rng)
        else:
            src = X[L - 1] if L != 9 else X[8]
            if fault == "swap_k" and L == 3:
                src = src.clone()
                src[:, [3, 4]] = src[:, [4, 3]]
            acc = _mm(src, Wl[:, :256].T.contiguous(), order, rng)
            if L in (5, 9):
                acc = acc + _mm(posx if L == 5 else posd, Wl[:, 256:].T.contiguous(), order, rng)
        acc = acc + b
        if RELU[L]:
            acc = torch.relu(acc)
        x = _store(acc, truncate=(fault == "truncate" and L == 2))
        if L == 9:
            x = torch.cat([x, torch.zeros(P, 128)], dim=1)
        X.append(x)
        masks.append(x != 0)
    sigma = _mm(X[7], Wt["sigma_fc.0.weight"].T.contiguous(), order, rng) + Wt["sigma_fc.0.bias"]
    rgb = _mm(X[9][:, :128], Wt["color_fc.2.weight"].T.contiguous(), order, rng) + Wt["color_fc.2.bias"]
    raw = torch.cat([rgb, sigma], dim=1)
    # the dX chain: d_raw enters it rounded to bf16; every stored dY is the next layer's operand
    dsr = torch.zeros(P, 32)
    dsr[:, :4] = d_raw.bfloat16().float()
    used = [m.clone() for m in masks]
    if fault == "flip_mask":
        p, f = [int(v) for v in torch.nonzero(~masks[4])[5]]
        used[4][p, f] = True
    dY = [None] * NUM_ACT
    for L in range(NUM_ACT - 1, -1, -1):
        if L == 9:
            acc = _mm(dsr[:, :3], Wt["color_fc.2.weight"].contiguous(), order, rng)
        elif L == 8:
            acc = _mm(dY[9][:, :128], Wt["color_fc.0.weight"][:, :256].contiguous(), order, rng)
        elif L == 7:
            acc = _mm(dY[8], Wt["layers_2.weight"].contiguous(), order, rng)
            if fault != "no_sigma":
                acc = acc + dsr[:, 3:4] @ Wt["sigma_fc.0.weight"]
        else:
            acc = _mm(dY[L + 1], Wt[LAYER_NAMES[L + 1] + ".weight"][:, :256].contiguous(), order, rng)
        if RELU[L]:
            acc = acc * used[L][:, :acc.shape[1]]
        y = _store(acc)
        if L == 9:
            y = torch.cat([y, torch.zeros(P, 128)], dim=1)
        dY[L] = y
    # the products over the points, into the flat vector with the leading dimensions of csrc/dw_gemm.hip
    grads = torch.zeros(PARAM_COUNT)
    nslab = (P + 31) // 32

    def product(name, A, B, col0=0, ldc=None, Nv=None, chunks=None):
        off, shape = OFFSETS[name]
        ldc = shape[1] if ldc is None else ldc
        C = _mm(A.T.contiguous(), B.contiguous(), "split" if order == "split" or chunks is not None else "plain", rng, chunks)
        Nv = B.shape[1] if Nv is None else Nv
        rows = torch.arange(A.shape[1])[:, None] * ldc
        cols = torch.arange(Nv)[None, :] + col0
        grads.index_put_(((off + rows + cols).reshape(-1),), C[:, :Nv].reshape(-1), accumulate=True)

    def bias(name, A, rows=None):
        off, shape = OFFSETS[name]
        A = A if rows is None else A[:rows]
        if order == "split":
            A = A[torch.from_numpy(rng.permutation(A.shape[0]))]
        grads[off:off + shape[0]] += A.sum(0)

    product("layers_0.0.weight", dY[0], posx64, Nv=64 if fault == "posx_leak" else 63)
    bias("layers_0.0.bias", dY[0])
    for L in (1, 2, 3, 4, 6, 7, 8):
        chunks = None
        if L == 2 and fault == "drop_slab":
            chunks = [s for s in range(nslab) if s != 2]
        if L == 3 and fault == "double_slab":
            chunks = list(range(nslab)) + [1]
        product(LAYER_NAMES[L] + ".weight", dY[L], X[L - 1], chunks=chunks)
        bias(LAYER_NAMES[L] + ".bias", dY[L], rows=(P - P % 32) if (L == 6 and fault == "bias_tail") else None)
    product("skip_conn_layer.0.weight", dY[5], X[4])
    product("skip_conn_layer.0.weight", dY[5], posx64, col0=255 if fault == "skip_col" else 256, Nv=63)
    bias("skip_conn_layer.0.bias", dY[5])
    product("sigma_fc.0.weight", dsr[:, 3:4], X[7])
    bias("sigma_fc.0.bias", d_raw[:, 3:4])
    product("color_fc.0.weight", dY[9][:, :128], X[8])
    product("color_fc.0.weight", dY[9][:, :128], posd32, col0=256, Nv=27)
    bias("color_fc.0.bias", dY[9][:, :128])
    product("color_fc.2.weight", dsr[:, :3], X[9][:, :128])
    bias("color_fc.2.bias", d_raw[:, :3])
    n = lambda t: t.numpy()
    return dict(X=[n(x) for x in X], masks=[n(m) for m in masks], raw=n(raw), dY=[n(y) for y in dY], dsr=n(dsr),
                d_raw=n(d_raw), posx=n(posx64), posd=n(posd32), grads=n(grads), P=P)
