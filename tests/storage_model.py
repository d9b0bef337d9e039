"""Host model of the 8-bit storage form of the training step (test infrastructure, after tests/train_chain_model.py, which
does the same for bf16): the documented layout (csrc/nerf_layout.h ``f8_*``, include/nerf_amd.h "8-bit storage form") restated
in numpy, in both directions, and crafted operands on which the products of csrc/dw_gemm_f8.hip must be EXACT.

  decode_e4m3_layers / decode_e4m3_narrow    device image -> values, bytes, exponent bytes
  encode_e4m3_layers / encode_e4m3_narrow    integer values + exponent bytes -> device image, everything else poisoned
  workgroup_shares                           the launchers' split of the workgroups over the products (the test sizes' source)
  crafted                                    integer operands under independently drawn power-of-two exponents, their images
                                             and the float64 gradient they must give

Why the crafted products are exact.  Operands are integers in [-2, 2] (exact in e4m3) under exponent bytes 126..128, so every
value is a multiple of 2^-1 of magnitude <= 4 and every product a multiple of MIN_PRODUCT = 2^-2 of magnitude <= MAX_PRODUCT =
16.  Inside one v_mfma_scale_f32_32x32x64_f8f6f4 a product is dropped only when it lies 2^-14 below the largest of its group of
eight (profiles/r04_f8_probe.txt, "sum inside one MFMA"): 16 / 2^-2 = 2^6 is far from that.  The instruction's sum is then added
to the accumulator by a true fp32 addition -- measured, profiles/f8_probe_accumulator.txt, "sum into the accumulator": C = 2^k
plus one product of 1.0 gives D - C = 1 for every k up to 23, and 0 (the tie, to even) at k = 24 -- so ``C + product`` is exact up
to the ratio ACCUMULATOR_EXACT_RATIO = R = 2^24.  Where, for every output entry, sum_p |a_p b_p| < R * MIN_PRODUCT, every partial
sum in any order (the instruction's, the accumulator's over the slabs, the float atomics of the split-K partials) is a multiple
of MIN_PRODUCT below 2^24 of them: representable, so nothing ever rounds.  ``crafted`` asserts exactly that, from the operand
range alone where it can (P * MAX_PRODUCT) and from the masses otherwise, lowering the density of nonzeros until it holds.

The same file records what the exponent byte 0xFF (e8m0's NaN) does: the instruction's result is NaN even where the block's
data bytes are all zero ("exponent byte 0xFF on K block 1").  A consumer must therefore never look at an exponent byte that no
producer wrote; the poison below puts 0xFF into every one of them.
"""
import numpy as np

import train_chain_model as M

E4M3 = np.array([np.nan if (v & 0x7f) == 0x7f else
                 (-1.0 if v & 0x80 else 1.0) * ((v & 7) / 8.0 * 2.0 ** -6 if (v >> 3) & 15 == 0 else (1 + (v & 7) / 8.0) * 2.0 ** (((v >> 3) & 15) - 7))
                 for v in range(256)])
# e4m3 byte of the integer v, index v + 16, for -16 <= v <= 16 (all exact: four significant bits)
INT_TO_E4M3 = np.array([next(b for b in range(256) if E4M3[b] == v and (v != 0 or b == 0)) for v in range(-16, 17)], dtype=np.uint8)
ACCUMULATOR_EXACT_RATIO = 2.0 ** 24          # R (module docstring; profiles/f8_probe_accumulator.txt)
EXP_BYTES = (126, 127, 128)                  # the crafted exponents: 2^-1, 2^0, 2^1
MAX_PRODUCT, MIN_PRODUCT = 16.0, 0.25
DATA_POISON, EXP_POISON, MASK_POISON = 0x7F, 0xFF, 0xFF      # e4m3 NaN; e8m0 NaN
PAD_VALUE = 7                                # pad columns inside a loaded chunk: finite, never an operand value
NARROW = ((64, 63), (32, 27), (16, 4))       # (width, true columns) of posx, posd and the packed d_raw, in scratch order
TILE, SLAB = 256, 64


def tiles(P):
    return (P + TILE - 1) // TILE


def blocks(P):
    return (P + 31) // 32


def align256(n):
    return (n + 255) // 256 * 256


# ---- sizes (nerf_layout.h) ---------------------------------------------------------------------------------------------
def f8_data_bytes(P):
    """The dY buffer: ten layers of 64 KiB per tile, then 8 exponent bytes per layer and 32-point block of every tile."""
    return 10 * tiles(P) * 65536 + 10 * tiles(P) * 64


def f8_acts_total_bytes(P):
    return align256(f8_data_bytes(P)) + 10 * tiles(P) * 8192


def narrow_bytes(W, P):
    return tiles(P) * (W // 16) * 4096 + tiles(P) * 64


def narrow_offsets(P):
    """({W: offset of the W-wide operand in the 8-bit scratch}, total bytes)."""
    off, out = 0, {}
    for W, _ in NARROW:
        out[W] = off
        off += align256(narrow_bytes(W, P))
    return out, off


# ---- decode ------------------------------------------------------------------------------------------------------------
def _per_element(exps, P, width):
    """[P, width] float64: 2^(byte - 127) of each element's (32-point block, 32-feature fragment)."""
    nq = (width + 31) // 32
    sc = 2.0 ** (exps[:, :nq].astype(np.float64) - 127.0)
    return np.repeat(np.repeat(sc, 32, axis=0)[:P], 32, axis=1)[:, :width]


def decode_e4m3_layers(host, P):
    """([10][P, 256] float64 values, [10][P, 256] bytes, [10][blocks, 8] exponent bytes) from the 8-bit buffer
    (nerf_layout.h f8_elem_offset / f8_scale_offset_bytes)."""
    nt = (P + 255) // 256
    vals, raws, exps = [], [], []
    scale0 = 10 * nt * 65536
    for L in range(10):
        blk = host[L * nt * 65536:(L + 1) * nt * 65536].reshape(nt, 16, 256, 16)
        b = blk.transpose(0, 2, 1, 3).reshape(nt * 256, 256)[:P]
        e = host[scale0 + L * nt * 64: scale0 + (L + 1) * nt * 64].reshape(nt * 8, 8)
        sc = 2.0 ** (e.astype(np.float64) - 127.0)                                    # [block, Q]
        per_elem = np.repeat(np.repeat(sc, 32, axis=0)[:P], 32, axis=1)               # [P, 256]
        vals.append(E4M3[b] * per_elem)
        raws.append(b)
        exps.append(e)
    return vals, raws, exps


def decode_e4m3_narrow(buf, W, P):
    """([P, W] float64 values, [P, W] bytes, [tiles * 8, 8] exponent bytes, [P, W] float64 2^(exponent - 127)) of one narrow
    operand (W in {64, 32, 16}; nerf_layout.h f8_narrow_*): ``buf`` starts at the operand."""
    nt = tiles(P)
    data_bytes = nt * (W // 16) * 4096
    blk = buf[:data_bytes].reshape(nt, W // 16, 256, 16).transpose(0, 2, 1, 3).reshape(nt * 256, W)[:P]
    e = buf[data_bytes:data_bytes + nt * 64].reshape(nt * 8, 8)
    per = _per_element(e, P, W)
    return E4M3[blk] * per, blk, e, per


def decode_scratch(scratch8, P):
    """{W: decode_e4m3_narrow(...)} of the three narrow operands of the 8-bit scratch."""
    offs, _ = narrow_offsets(P)
    return {W: decode_e4m3_narrow(scratch8[offs[W]:], W, P) for W, _ in NARROW}


# ---- encode ------------------------------------------------------------------------------------------------------------
def encode_e4m3_layers(values, exp_bytes, P, data_fill=DATA_POISON, exp_fill=EXP_POISON):
    """values int8 [10, P, 256] (integers in [-16, 16]), exp_bytes uint8 [10, blocks(P), 8] -> the 8-bit buffer, uint8
    [f8_data_bytes(P)].  ``data_fill``: the data bytes of points >= P in the last tile and of layer 9's chunks 8..15 (features
    past its width); ``exp_fill``: the exponent bytes of blocks with no point and of layer 9's fragments 4..7."""
    nt, nb = tiles(P), blocks(P)
    assert values.shape == (10, P, 256) and exp_bytes.shape == (10, nb, 8)
    data = np.full((10, nt * 256, 256), data_fill, dtype=np.uint8)
    data[:, :P] = INT_TO_E4M3[values.astype(np.int16) + 16]
    data[9, :, 128:] = data_fill
    blocked = data.reshape(10, nt, 256, 16, 16).transpose(0, 1, 3, 2, 4)              # [L][tile][chunk][point][16]
    exps = np.full((10, nt * 8, 8), exp_fill, dtype=np.uint8)
    exps[:, :nb] = exp_bytes
    exps[9, :, 4:] = exp_fill
    return np.concatenate([np.ascontiguousarray(blocked).reshape(-1), exps.reshape(-1)])


def acts_image(encoded, P, mask_fill=MASK_POISON):
    """The activation buffer around ``encode_e4m3_layers``' bytes: the alignment gap and the ReLU mask region (no operand of
    the products) at ``mask_fill``."""
    out = np.full(f8_acts_total_bytes(P), mask_fill, dtype=np.uint8)
    out[:encoded.size] = encoded
    return out


def encode_e4m3_narrow(values, exp_bytes, W, P, data_fill=DATA_POISON, exp_fill=EXP_POISON):
    """values [P, W] integers, exp_bytes uint8 [blocks(P), ceil(W / 32)] -> one narrow operand, uint8 [narrow_bytes(W, P)]."""
    nt, nb, nq = tiles(P), blocks(P), (W + 31) // 32
    assert values.shape == (P, W) and exp_bytes.shape == (nb, nq)
    data = np.full((nt * 256, W), data_fill, dtype=np.uint8)
    data[:P] = INT_TO_E4M3[values.astype(np.int16) + 16]
    blocked = data.reshape(nt, 256, W // 16, 16).transpose(0, 2, 1, 3)
    exps = np.full((nt * 8, 8), exp_fill, dtype=np.uint8)
    exps[:nb, :nq] = exp_bytes
    return np.concatenate([np.ascontiguousarray(blocked).reshape(-1), exps.reshape(-1)])


def scratch_image(narrow_ints, narrow_exps, P, fill=EXP_POISON):
    """The 8-bit scratch: the three narrow operands at their offsets, the gaps at ``fill``."""
    offs, total = narrow_offsets(P)
    out = np.full(total, fill, dtype=np.uint8)
    for W, _ in NARROW:
        img = encode_e4m3_narrow(narrow_ints[W], narrow_exps[W], W, P)
        out[offs[W]:offs[W] + img.size] = img
    return out


# ---- the launchers' arithmetic (csrc/dw_products.h dw_plan; checked against it by tests/test_dw_products_cpu.py) --------------
# (features of A + features of B, head of the flat vector?) of the 14 products in table order, in the e4m3 form
PRODUCT_WIDTHS = ((256 + 64, True), (512, True), (512, True), (512, True), (512, True), (512, False), (256 + 64, False),
                  (512, False), (512, False), (16 + 256, False), (512, False), (128 + 256, False), (128 + 32, False),
                  (16 + 128, False))
DRAW_PRODUCTS = (9, 13)                      # the products whose A operand is the packed d_raw: the 16 above, 32 in the bf16 form
SLAB_COST = 1024.0
# what a storage form brings to the arithmetic: points per slab, operand bytes per feature, features of the packed d_raw
E4M3_FORM = dict(slab=SLAB, bytes_per_feature=1, draw=16)        # the defaults below
BF16_FORM = dict(slab=32, bytes_per_feature=2, draw=32)


def product_widths(draw=16):
    """PRODUCT_WIDTHS with the packed d_raw ``draw`` features wide."""
    return tuple((w + (draw - 16 if i in DRAW_PRODUCTS else 0), head) for i, (w, head) in enumerate(PRODUCT_WIDTHS))


def ideal_shares(bucket, cus=256, draw=16):
    """The workgroups each product of the launch would get with slabs to spare: cus * (M + N + 1024) / sum of the same."""
    w = [float(a + SLAB_COST) for a, head in product_widths(draw) if bucket == 0 or head == (bucket == 2)]
    return [x / sum(w) * cus for x in w]


def workgroup_shares(P, bucket, cus=256, slab=SLAB, bytes_per_feature=1, draw=16):
    """[wgs of each product of the launch] for P points: the integer parts of the ideal shares, at least ``need`` (a slice's
    operand stays below 1 GiB), at most one workgroup per slab, the workgroups left over by largest remainder."""
    nslab = (P + slab - 1) // slab
    need = (P * 256 * bytes_per_feature >> 30) + 1
    w, rem = [], []
    for share in ideal_shares(bucket, cus, draw):
        wi, ri = int(share), share - int(share)
        if wi < need:
            wi, ri = need, 0.0
        if wi >= nslab:
            wi, ri = nslab, -1.0
        w.append(wi)
        rem.append(ri)
    used = sum(w)
    while used < cus:
        best = -1
        for i in range(len(w)):
            if rem[i] >= 0 and w[i] < nslab and (best < 0 or rem[i] > rem[best]):
                best = i
        if best < 0:
            break
        w[best] += 1
        rem[best] = 0.0
        used += 1
    return w


def clamp_binds(P, bucket, cus=256, slab=SLAB, bytes_per_feature=1, draw=16):
    """Does ``need`` raise a share, or the slab count stop one (before or after its leftover workgroup)?  Where neither
    happens the shares add up to ``cus``."""
    nslab = (P + slab - 1) // slab
    need = (P * 256 * bytes_per_feature >> 30) + 1
    return any(int(s) < need or int(s) + 1 >= nslab for s in ideal_shares(bucket, cus, draw))


def share_edge_sizes(cus=256, slab=SLAB, bytes_per_feature=1, draw=16):
    """For each of the three launches (bucket 0, 1, 2) and for its smallest and its largest per-product share w: the sizes with
    w - 1, w and w + 1 slabs, each one point short of, at and one point past the slab boundary."""
    out = set()
    for bucket in (0, 1, 2):
        sh = workgroup_shares(1 << 20, bucket, cus, slab, bytes_per_feature, draw)    # slabs to spare: the shares no clamp has touched
        for w in (min(sh), max(sh)):
            for s in (w - 1, w, w + 1):
                out.update((slab * s - 1, slab * s, slab * s + 1))
    return sorted(out)


# 1 .. 97: blocks and slabs -- one point, a block one short / full / one over, a slab likewise, a slab whose second block is
#   absent (1, 31, 32, 65, 95, 96: odd block counts) or ragged (33, 63, 97), always fewer slabs than workgroups;
# 255, 256, 257: tile edges;
# share_edge_sizes(): "slabs == workgroups of this product" and one slab either side of it, for the smallest and the largest
#   share of each launch (bucket 0: 15 and 20 workgroups, bucket 1: 24 and 31, bucket 2: 46 and 53, for 256 CUs) -- where
#   s_begin / s_end, the vmcnt ladder and ``left`` take their edge values (a workgroup with one slab, with two, a product
#   clamped to one workgroup per slab);
# 2405: ragged, several slabs per workgroup; 36,928 = 577 slabs: the ring in steady state, 145 tiles (about 100 MB per buffer).
# (the ``need`` clamp -- more than 2^22 points, 1 GiB per operand -- is out of reach of a GPU test that stays quick; the
# arithmetic itself is run there on the host: tests/test_dw_products_cpu.py.)
SMALL_SIZES = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 255, 256, 257)
INT_SIZES = tuple(sorted(set(SMALL_SIZES) | set(share_edge_sizes()) | {2405, 36928}))


# ---- crafted operands ----------------------------------------------------------------------------------------------------
class Scaled:
    """The ten layers of an int8 operand under their exponents, converted to float64 one at a time."""

    def __init__(self, ints, exps, P):
        self.ints, self.exps, self.P = ints, exps, P

    def __getitem__(self, L):
        return self.ints[L].astype(np.float64) * _per_element(self.exps[L], self.P, 256)


def _draw_exps(rng, shape):
    e = rng.choice(np.array(EXP_BYTES, dtype=np.uint8), size=shape)
    # selectivity by construction (tests/test_storage_model_cpu.py), on top of the independent draws: in block 0 fragments 0
    # and 1 differ (a kernel that reads byte Q ^ 1 is seen even with one block), and blocks 0 and 1 differ in fragment 0 (one
    # that swaps the two blocks of a slab is seen even with one slab and one fragment)
    lo, n = EXP_BYTES[0], len(EXP_BYTES)
    other = (lo + (e[..., 0, 0].astype(np.int64) - lo + 1) % n).astype(np.uint8)      # a different byte than e[..., 0, 0]
    if e.shape[-1] > 1:
        e[..., 0, 1] = np.where(e[..., 0, 1] == e[..., 0, 0], other, e[..., 0, 1])
    if e.shape[-2] > 1:
        e[..., 1, 0] = np.where(e[..., 1, 0] == e[..., 0, 0], other, e[..., 1, 0])
    return e.astype(np.uint8)


def narrow_entries(y, X, dY, posx, posd, dsr, d_raw):
    """Overwrite, in the flat gradient ``y``, the entries that the narrow operands enter (float64 values [P, >= true columns])."""
    def put(name, cols, v):
        off, shape = M.OFFSETS[name]
        y[off:off + int(np.prod(shape))].reshape(shape)[:, cols] = v

    posx, posd = posx[:, :63], posd[:, :27]
    put("layers_0.0.weight", slice(0, 63), dY[0].T @ posx)
    put("skip_conn_layer.0.weight", slice(256, 319), dY[5].T @ posx)
    put("color_fc.0.weight", slice(256, 283), dY[9][:, :128].T @ posd)
    put("sigma_fc.0.weight", slice(0, 256), dsr[:, 3:4].T @ X[7])
    put("color_fc.2.weight", slice(0, 128), dsr[:, :3].T @ X[9][:, :128])
    for name, v in (("sigma_fc.0.bias", d_raw[:, 3:4].sum(0)), ("color_fc.2.bias", d_raw[:, :3].sum(0))):
        off, shape = M.OFFSETS[name]
        y[off:off + shape[0]] = v
    return y


def crafted(P, seed, density=1.0):
    """Integer operands in [-2, 2] (a fraction ``density`` of them drawn, the rest zero) under exponent bytes drawn independently
    per (layer, 32-point block, fragment Q) from EXP_BYTES, the device images that hold them in poisoned surroundings, and the
    float64 gradients they must give.  Returns a dict:

      ints     'X', 'dY' int8 [10, P, 256]; 64, 32, 16: int8 [P, W] (pad columns PAD_VALUE); 'd_raw' float32 [P, 4]
      exps     'X', 'dY' uint8 [10, blocks, 8]; 64, 32, 16: uint8 [blocks, ceil(W / 32)]
      acts, dys, scratch8      the device images (uint8)
      want_crafted             the flat gradient for the crafted narrow images (their own exponents; head biases from d_raw)
      want_converted           the same with the narrow operands at exponent 0: what integer bf16 rows and an integer d_raw
                               give through nerf_amd_param_gradients_convert_e4m3 (d_raw = the packed operand's columns 0..3)
      density                  the density used (lowered until the exactness assertion of the module docstring holds)
      largest_mass             an upper bound of sum_p |a_p b_p| over the output entries: below R * MIN_PRODUCT
    """
    nb = blocks(P)
    f8 = np.float64
    while True:
        rng = np.random.Generator(np.random.PCG64(seed))
        ints, exps = {}, {}
        for name in ("X", "dY"):
            v = rng.integers(-2, 3, size=(10, P, 256), dtype=np.int8)
            if density < 1.0:
                v *= rng.random(size=v.shape) < density
            v[9, :, 128:] = 0                              # past layer 9's width: not an operand (data poison in the image)
            ints[name] = v
            exps[name] = _draw_exps(rng, (10, nb, 8))
        for W, true in NARROW:
            v = rng.integers(-2, 3, size=(P, W), dtype=np.int8)
            if density < 1.0:
                v *= rng.random(size=v.shape) < density
            if W == 16:
                v[P - 1, :true][v[P - 1, :true] == 0] = 1  # the last point carries every row of d_raw (a lone last slab is seen)
            v[:, true:] = PAD_VALUE
            ints[W] = v
            exps[W] = _draw_exps(rng, (nb, (W + 31) // 32))
        ints["d_raw"] = ints[16][:, :4].astype(np.float32)
        X, dY = Scaled(ints["X"], exps["X"], P), Scaled(ints["dY"], exps["dY"], P)
        nar = {W: ints[W].astype(f8) * _per_element(exps[W], P, W) for W, _ in NARROW}
        d_raw = ints["d_raw"].astype(f8)
        # the exactness assertion: sum_p |a_p b_p| < R * MIN_PRODUCT for every output entry -- from the operand range alone
        # where that is enough, from the masses otherwise
        largest_mass = P * MAX_PRODUCT
        if largest_mass < ACCUMULATOR_EXACT_RATIO * MIN_PRODUCT:
            want, _ = M.expected_param_grads(X, dY, nar[64], nar[32], nar[16], d_raw, with_mass=False)
            break
        want, mass = M.expected_param_grads(X, dY, nar[64], nar[32], nar[16], d_raw)
        largest_mass = float(mass.max())
        if largest_mass < ACCUMULATOR_EXACT_RATIO * MIN_PRODUCT:
            break
        density *= 0.5
    assert np.array_equal(want, np.round(want / MIN_PRODUCT) * MIN_PRODUCT)
    plain = {W: ints[W].astype(f8) for W, _ in NARROW}
    want_converted = narrow_entries(want.copy(), X, dY, plain[64], plain[32], plain[16], d_raw)
    enc = {k: encode_e4m3_layers(ints[k], exps[k], P) for k in ("X", "dY")}
    return dict(P=P, ints=ints, exps=exps, acts=acts_image(enc["X"], P), dys=enc["dY"], scratch8=scratch_image(ints, exps, P),
                want_crafted=want, want_converted=want_converted, density=density, largest_mass=largest_mass)


# ---- what a subtly wrong kernel would compute ----------------------------------------------------------------------------
# the products of the launcher's table as (A operand, its columns, B operand, its columns); a bias sum has B = None
def _product_table():
    t = [(("dY", 0), 256, (64,), 63)]
    t += [(("dY", l), 256, ("X", l - 1), 256) for l in (1, 2, 3, 4)]
    t += [(("dY", 5), 256, ("X", 4), 256), (("dY", 5), 256, (64,), 63), (("dY", 6), 256, ("X", 5), 256),
          (("dY", 7), 256, ("X", 6), 256), ((16,), slice(3, 4), ("X", 7), 256), (("dY", 8), 256, ("X", 7), 256),
          (("dY", 9), 128, ("X", 8), 256), (("dY", 9), 128, (32,), 27), ((16,), slice(0, 3), ("X", 9), 128)]
    t += [(("dY", l), 128 if l == 9 else 256, None, None) for l in range(10)]
    return t


PRODUCTS = _product_table()
VARIANTS = ("swap_q", "swap_blocks", "drop_first_slab", "drop_last_slab")


def _operand(c, key, exps=None, width=None):
    """(integers [P, W] float32, 2^(exponent - 127) per element [P, W] float32) of operand ``key`` = ('X' | 'dY', L) or (W,),
    the first ``width`` features of it.  (float32 holds these values and every sum of their products exactly: crafted().)"""
    if len(key) == 2:
        v, e, W = c["ints"][key[0]][key[1]], c["exps"][key[0]][key[1]], 256
    else:
        v, e, W = c["ints"][key[0]], c["exps"][key[0]], key[0]
    W = W if width is None else min(W, width)
    return v[:, :W].astype(np.float32), _per_element(e if exps is None else exps, c["P"], W).astype(np.float32)


def _cols(a, sel):
    return a[:, sel] if isinstance(sel, slice) else a[:, :sel]


def variant_changes(c, variant, max_features=None):
    """{(product index, operand key): largest |change| of the product's entries} when the kernel misreads the crafted images
    in one way, for every product and every operand of it the variant applies to:

      swap_q           the exponent bytes Q and Q ^ 1 of the operand swapped in every block (the wrong byte of a group of four)
      swap_blocks      the exponent bytes of the two blocks of every slab swapped (block 1's exponent on lanes 0..31)
      drop_first_slab / drop_last_slab     one 64-point slab of the product missing (key None: both operands)

    ``max_features``: look at the first so many features of the misread operand only (a change there is a change)."""
    P, nb = c["P"], blocks(c["P"])
    out, memo = {}, {}

    def value(key):
        if key not in memo:
            if P > 8192:
                memo.clear()                       # one operand at a time at the large size
            memo[key] = np.multiply(*_operand(c, key))
        return memo[key]

    drop = variant.startswith("drop")
    pts = slice(0, P)
    if drop:
        pts = slice(0, min(SLAB, P)) if variant == "drop_first_slab" else slice((P - 1) // SLAB * SLAB, P)
    for i, (ka, ca, kb, cb) in enumerate(PRODUCTS):
        A = _cols(value(ka)[pts], ca)
        B = np.ones((pts.stop - pts.start, 1), dtype=np.float32) if kb is None else _cols(value(kb)[pts], cb)
        if drop:
            out[(i, None)] = float(np.abs(A.T @ B).max())
            continue
        for side, key in ((0, ka), (1, kb)):
            if key is None:
                continue
            e = (c["exps"][key[0]][key[1]] if len(key) == 2 else c["exps"][key[0]]).copy()
            if variant == "swap_q":
                if e.shape[1] < 2:
                    continue                       # one fragment: byte Q ^ 1 lies past the width (poisoned: NaN, seen anyway)
                e = e.reshape(nb, -1, 2)[:, :, ::-1].reshape(nb, -1)
            else:
                if nb < 2:
                    continue                       # one block: nothing to swap with (block 1's bytes are poisoned)
                full = nb // 2 * 2
                e[:full] = e[:full].reshape(-1, 2, e.shape[1])[:, ::-1].reshape(full, e.shape[1])
            v, s_wrong = _operand(c, key, e, max_features)
            _, s_right = _operand(c, key, None, max_features)
            D = _cols(v * (s_wrong - s_right), ca if side == 0 else cb)
            out[(i, key)] = float(np.abs(D.T @ B if side == 0 else A.T @ D).max())
    return out
