"""GPU tests that pin every positional-encoder feature of the fused kernels to float64 (tests/encoder_probe_model.py; DESIGN.md
"Encoder probe").

The 16-bit kernels form the 63 + 27 features in registers with the hardware sine (csrc/nerf_device.h to_revolutions +
enc_lane); probe weight sets -- one-hot taps, identity layers behind them -- turn single features into outputs, exact in
the operand type, so that each one is compared with float64 sin / cos (2^l x) by the interval check
round_T(ref - E) <= got <= round_T(ref + E).  Per kernel path the largest EXCESS (distance from the float64 value to the
rounding cell of what came back: the encoder's own error as far as a 16-bit readout shows it) is printed per entry point,
level and trig; nothing here compares a kernel with another kernel, except the composition test at the end.

  points path   nerf_amd_mlp_forward fp16 / bf16 / fp32, nerf_amd_mlp_forward_train_points (bf16): the sweeps of the model,
                P = 1, 255, 256, 257, 515 into sentinel-padded outputs;
  rays path     nerf_amd_mlp_forward_rays fp16 / bf16 / fp32 and nerf_amd_mlp_forward_train with explicit positions: one
                direction slot per ray of a tile, tile seams inside rays, every ray a direction of its own; the float64
                reference is taken on the points nerf_amd_query_points forms from the same rays (the same fetch code);
  density       nerf_amd_density_forward fp16 / bf16, rows of 3 and of 6 floats, the 126 posx taps on sigma;
  stored rows   nerf_amd_encode_points_bf16 / nerf_amd_sample_encode_bf16 directly (sincos_rev_fast), pad columns zero;
  composition   nerf_amd_render_forward == nerf_amd_mlp_forward_rays + nerf_amd_volume_render_rays on probe weights, bit for
                bit as tests/test_gpu_parity.py::test_fused_render_equals_two_launch_path asserts it.

The asserted allowances are encoder_probe_model.E_FAST (in-register features, enc_lane) and E_ROWS (stored rows,
sincos_rev_fast): twice the measured maximum, rounded up to one digit, never above the project's 2e-6 (provenance next to
the constants); the fp32 kernels use the exact encoder and are held to ENC_ATOL.  Measured maxima: enc_lane paths 5.58e-7
(fp16) / 5.56e-7 (bf16) on every sweep up to |x| = 4096, stored rows 3.74e-7, fp32 6.8e-8.
"""
import numpy as np
import pytest
import torch

import encoder_probe_model as M

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
ROW_SENTINEL = 776.0                       # the stored rows are bf16: a sentinel that bf16 holds
RAGGED_P = (1, 255, 256, 257, 2 * 256 + 3)
RAY_SHAPES = ((300, 1), (90, 3), (20, 40), (7, 64), (3, 257))       # a 256-point tile holds 256, ~86, ~7, 4 and < 1 rays
OPERAND = {"fp16": "fp16", "bf16": "bf16", "fp32": "fp32", "train": "bf16"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with a GPU: pytest -m gpu"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


class Probes:
    """The probe weight sets on the device, packed on first use per precision."""

    def __init__(self, dev, synthetic):
        from nerf_simple_amd import _lib
        self.dev, self.L, self.lib = dev, _lib, _lib.lib()
        self.flat, self.taps, self.images = {}, {}, {}
        for sigma_only in (False, True):
            sets = list(M.probe_weight_sets(sigma_only))
            self.flat[sigma_only] = [synthetic.flatten_state_dict(sd).to(dev) for sd, _ in sets]
            self.taps[sigma_only] = [taps for _, taps in sets]

    def code(self, path):
        return self.L.precision_code("bf16" if path == "train" else path)

    def packed(self, s, path, sigma_only=False):
        code = self.code(path)
        key = (s, code, sigma_only)
        if key not in self.images:
            buf = torch.empty(self.lib.nerf_amd_packed_bytes(code), dtype=torch.uint8, device=self.dev)
            self.L.check(self.lib.nerf_amd_pack_weights(self.L.ptr(self.flat[sigma_only][s]), self.L.ptr(buf), code,
                                                        self.L.stream_ptr(self.dev)), "nerf_amd_pack_weights")
            self.images[key] = buf
        return self.images[key]

    def status(self, packed, path):
        """(non-finite value seen, weight out of range) of a 16-bit image."""
        off = int(self.lib.nerf_amd_packed_status_offset(self.code(path)))
        w = packed[off:off + 8].view(torch.int32).cpu()
        return int(w[0]), int(w[1])

    def clear_status(self, packed, path):
        off = int(self.lib.nerf_amd_packed_status_offset(self.code(path)))
        packed[off:off + 8].zero_()


@pytest.fixture(scope="module")
def probes(dev, synthetic):
    return Probes(dev, synthetic)


class Table:
    """Largest excess per (entry, level, trig) of one kernel path; failures of the interval check with their inputs."""

    def __init__(self, name, E=M.E_FAST):
        self.name, self.E, self.worst, self.fail = name, E, {}, []

    def check(self, got, refs, taps, T, src, note=""):
        """got [P, 4] outputs of one weight set; refs {entry: [P, columns] float64}; src {entry: [P, 3] inputs}."""
        tapped = {ch for ch, _, _ in taps}
        for ch in range(got.shape[1]):
            if ch not in tapped and got[:, ch].any():
                self.fail.append(f"{note} untapped output {ch} is not zero")
        for ch, entry, col in taps:
            c, level, trig = M.column_info(entry, col)
            ref = refs[entry][:, col]
            E = 0.0 if level < 0 else (M.ENC_ATOL if T == "fp32" else self.E)
            ok, ex = M.interval_check(got[:, ch], ref, T, E, fp16_flush=M.FP16_OPERANDS_FLUSH)
            key = (entry, level, trig)
            self.worst[key] = max(self.worst.get(key, 0.0), float(ex.max()) if len(ex) else 0.0)
            if not ok.all():
                i = int(np.argmax(np.where(ok, -1.0, ex + 1e-300)))
                self.fail.append(f"{note} {entry} column {col} (coordinate {c}, level {level}, trig {trig}) -> output {ch}: "
                                 f"{int((~ok).sum())} of {len(ok)} outside, worst at x = {src[entry][i, c]!r}: ref {ref[i]:.9e} "
                                 f"got {got[i, ch]:.9e} excess {ex[i]:.3e}")

    def report(self):
        for entry in ("l0", "skip", "posd"):
            keys = sorted(k for k in self.worst if k[0] == entry)
            if not keys:
                continue
            raw = self.worst.get((entry, -1, 0), 0.0)
            trig_keys = [k for k in keys if k[1] >= 0]
            if trig_keys:
                top = max(self.worst[k] for k in trig_keys)
                rows = " ".join(f"{k[1]}{'sc'[k[2]]}={self.worst[k]:.2e}" for k in trig_keys)
                print(f"{self.name} {entry}: max excess {top:.3e} raw {raw:.1e} | {rows}")
            else:
                print(f"{self.name} {entry}: raw {raw:.1e}")
        return max([v for k, v in self.worst.items() if k[1] >= 0], default=0.0)

    def finish(self):
        top = self.report()
        assert not self.fail, f"{self.name}: {len(self.fail)} failures\n" + "\n".join(self.fail[:12])
        return top


def _refs(pts64):
    """float64 reference columns of the three entry points for query points [P, 6] (float64 of the kernels' fp32 inputs)."""
    x, d = pts64[:, :3], pts64[:, 3:]
    rx = M.ref_rows(x, "l0")
    return {"l0": rx, "skip": rx, "posd": M.ref_rows(d, "posd")}, {"l0": x, "skip": x, "posd": d}


_REF_CACHE = {}


def _sweep(lim):
    """(fp32 sweep points [S, 6], their float64 references) -- computed once per limit."""
    if lim not in _REF_CACHE:
        pts = M.sweep_points(lim)
        _REF_CACHE[lim] = (pts,) + _refs(pts.astype(np.float64))
    return _REF_CACHE[lim]


def _slice(refs, src, lo, hi):
    return {k: v[lo:hi] for k, v in refs.items()}, {k: v[lo:hi] for k, v in src.items()}


def _forward_points(pr, path, packed, v, P, pad=64):
    """out[P + pad, 4] (sentinel-filled) of the points-mode kernel of `path` on the first P rows of v."""
    L, lib, dev = pr.L, pr.lib, pr.dev
    out = torch.full((P + pad, 4), SENTINEL, device=dev)
    if path == "train":
        acts = torch.empty(int(lib.nerf_amd_train_activation_bytes(P)), dtype=torch.uint8, device=dev)
        L.check(lib.nerf_amd_mlp_forward_train_points(L.ptr(v), L.ptr(packed), L.ptr(out), L.ptr(acts), P, L.stream_ptr(dev)),
                "nerf_amd_mlp_forward_train_points")
    else:
        L.check(lib.nerf_amd_mlp_forward(L.ptr(v), L.ptr(packed), L.ptr(out), P, pr.code(path), L.stream_ptr(dev)),
                "nerf_amd_mlp_forward")
    return out


def _run_points(pr, path, lim, sizes, table):
    pts, refs, src = _sweep(lim)
    T = OPERAND[path]
    S = len(pts)
    for P in sizes:
        lo = 0 if P == S else (37 * P) % (S - P)                     # ragged sizes look at different parts of the sweep
        v = torch.from_numpy(pts[lo:lo + P].copy()).to(pr.dev).contiguous()
        r, x = _slice(refs, src, lo, lo + P)
        outs = [_forward_points(pr, path, pr.packed(s, path), v, P) for s in range(len(pr.taps[False]))]
        host = torch.stack(outs).cpu().numpy()
        for s, taps in enumerate(pr.taps[False]):
            assert (host[s, P:] == SENTINEL).all(), (path, P, s, "wrote past the last point")
            table.check(host[s, :P].astype(np.float64), r, taps, T, x, note=f"P={P} set {s}")


# ---- points path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fp16", "bf16", "fp32", "train"])
def test_points_path_scene_range(dev, probes, path):
    """Every tap through the points-mode kernel on the scene-range sweep (|x| <= 4.5, in points mode the direction columns
    carry the whole sweep too) and on the ragged sizes around the 256-point tile (128 in fp32)."""
    table = Table(f"points {path} lim=4.5")
    _run_points(probes, path, 4.5, (len(M.sweep_points(4.5)),) + RAGGED_P, table)
    top = table.finish()
    if path != "fp32":
        # sanity print, not a gate: the measured total cannot sit far below the arithmetic part alone
        print(f"points {path}: measured {top:.3e} against the emulated arithmetic-only error {M.ARITH_BOUND:.1e}")
        for packed_key, buf in probes.images.items():
            if packed_key[1] == probes.code(path):
                assert probes.status(buf, path) == (0, 0), packed_key


@pytest.mark.parametrize("lim", [64.0, 4096.0])
@pytest.mark.parametrize("path", ["fp16", "bf16"])
def test_points_path_wide_sweeps(dev, probes, path, lim):
    """The same beyond the scene: |x| up to 64 and up to 4096 (the documented domain of the allowance, include/nerf_amd.h)."""
    table = Table(f"points {path} lim={lim:g}")
    _run_points(probes, path, lim, (len(M.sweep_points(lim)),), table)
    table.finish()


def test_fp16_subnormal_operands(dev, probes):
    """Whether an fp16 subnormal operand survives the MFMA path, recorded in encoder_probe_model.FP16_OPERANDS_FLUSH (DESIGN.md
    "Encoder probe"): the raw-column taps at |x| < 2^-14."""
    pts, refs, src = _sweep(4.5)
    v = torch.from_numpy(pts.copy()).to(dev).contiguous()
    seen = kept = 0
    for s, taps in enumerate(probes.taps[False]):
        raws = [(ch, e, j) for ch, e, j in taps if j < 3]
        if not raws:
            continue
        got = _forward_points(probes, "fp16", probes.packed(s, "fp16"), v, len(pts))[:len(pts)].cpu().numpy().astype(np.float64)
        for ch, e, j in raws:
            want = M.round_to(refs[e][:, j], "fp16")
            sub = (np.abs(want) < M.FP16_MIN_NORMAL) & (want != 0)
            seen += int(sub.sum())
            kept += int((got[sub, ch] == want[sub]).sum())
    print(f"fp16 subnormal operands: {kept} of {seen} came back as rounded (the rest flushed or wrong)")
    assert seen > 0
    assert kept == (0 if M.FP16_OPERANDS_FLUSH else seen)


# ---- rays path ----------------------------------------------------------------------------------------------------------------
def _query_points(pr, rays, ts, B, N):
    L, lib, dev = pr.L, pr.lib, pr.dev
    q = torch.empty(B * N, 6, device=dev)
    L.check(lib.nerf_amd_query_points(L.ptr(rays), L.ptr(ts), None, L.FLAG_TS_GIVEN, 0, 0, L.ptr(q), None, B, N,
                                      L.stream_ptr(dev)), "nerf_amd_query_points")
    return q.cpu().numpy()


def _forward_rays(pr, path, packed, rays, ts, B, N, pad=16):
    """(raw [B * N + pad, 4] sentinel-filled, ts_out [B, N]) of the rays-mode kernel of `path` with explicit positions."""
    L, lib, dev = pr.L, pr.lib, pr.dev
    raw = torch.full((B * N + pad, 4), SENTINEL, device=dev)
    ts_out = torch.full((B, N), SENTINEL, device=dev)
    if path == "train":
        acts = torch.empty(int(lib.nerf_amd_train_activation_bytes(B * N)), dtype=torch.uint8, device=dev)
        L.check(lib.nerf_amd_mlp_forward_train(L.ptr(rays), L.ptr(ts), None, L.ptr(packed), L.FLAG_TS_GIVEN, 0, 0, L.ptr(raw),
                                               L.ptr(ts_out), L.ptr(acts), B, N, L.stream_ptr(dev)), "nerf_amd_mlp_forward_train")
    else:
        L.check(lib.nerf_amd_mlp_forward_rays(L.ptr(rays), L.ptr(ts), None, L.ptr(packed), pr.code(path), L.FLAG_TS_GIVEN, 0, 0,
                                              L.ptr(raw), L.ptr(ts_out), B, N, L.stream_ptr(dev)), "nerf_amd_mlp_forward_rays")
    return raw, ts_out


def _ray_case(case):
    """rays, ts (numpy) of a case: a (B, N) of RAY_SHAPES, or 'sweep' = the scene-range value sweep as origins, N = 1."""
    if case == "sweep":
        B, N = len(M.sweep_points(4.5)), 1
        return (B, N) + M.probe_rays(B, N, lim=4.5)
    B, N = case
    return (B, N) + M.probe_rays(B, N)


@pytest.mark.parametrize("case", RAY_SHAPES + ("sweep",), ids=lambda c: c if isinstance(c, str) else f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("path", ["fp16", "bf16", "fp32", "train"])
def test_rays_path(dev, probes, path, case):
    """Every tap through the rays-mode kernels.  The inference instantiations evaluate the direction features once per ray
    of the tile into an LDS slot (RAY_POSD): every ray has a direction of its own, so a slot read for the wrong ray at a
    tile seam lands outside its interval.  Only `raw` and `ts` are looked at (N = 1 included)."""
    B, N, rays_h, ts_h = _ray_case(case)
    rays = torch.from_numpy(rays_h).to(dev).contiguous()
    ts = torch.from_numpy(ts_h).to(dev).contiguous()
    q = _query_points(probes, rays, ts, B, N)
    refs, src = _refs(q.astype(np.float64))
    unit = rays_h[:, 3:].astype(np.float64)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    assert np.abs(q[:, 3:].reshape(B, N, 3) - unit[:, None, :]).max() <= 2e-7           # the directions are the rays' own
    table = Table(f"rays {path} {B}x{N}")
    outs = []
    for s in range(len(probes.taps[False])):
        raw, ts_out = _forward_rays(probes, path, probes.packed(s, path), rays, ts, B, N)
        outs.append(raw)
        if s == 0:
            assert torch.equal(ts_out, ts)
    host = torch.stack(outs).cpu().numpy()
    for s, taps in enumerate(probes.taps[False]):
        assert (host[s, B * N:] == SENTINEL).all(), (path, case, s, "wrote past the last point")
        table.check(host[s, :B * N].astype(np.float64), refs, taps, OPERAND[path], src, note=f"set {s}")
    table.finish()


# ---- the sigma-only kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [3, 6])
@pytest.mark.parametrize("path", ["fp16", "bf16"])
def test_density_kernel(dev, probes, path, stride):
    """nerf_amd_density_forward forms posx in a prologue of its own: all 126 posx taps (both entries) on sigma, rows of three
    and of six floats, the scene-range sweep and the ragged sizes."""
    L, lib = probes.L, probes.lib
    pts, refs, src = _sweep(4.5)
    S = len(pts)
    table = Table(f"density {path} stride {stride}")
    nsets = len(probes.taps[True])
    for P in (S,) + RAGGED_P:
        lo = 0 if P == S else (53 * P) % (S - P)
        v = torch.from_numpy(np.ascontiguousarray(pts[lo:lo + P, :stride])).to(dev).contiguous()
        r, x = _slice(refs, src, lo, lo + P)
        sig = torch.full((nsets, P + 64), SENTINEL, device=dev)
        for s in range(nsets):
            L.check(lib.nerf_amd_density_forward(L.ptr(v), stride, L.ptr(probes.packed(s, path, True)), probes.code(path),
                                                 L.ptr(sig[s]), P, L.stream_ptr(dev)), "nerf_amd_density_forward")
        host = sig.cpu().numpy()
        assert (host[:, P:] == SENTINEL).all(), (path, stride, P, "wrote past the last point")
        for s, taps in enumerate(probes.taps[True]):
            table.check(host[s, :P, None].astype(np.float64), r, [(0, taps[0][1], taps[0][2])], path, x, note=f"P={P} set {s}")
    table.finish()


# ---- the stored bf16 rows ---------------------------------------------------------------------------------------------------
def _check_rows(table, px, pd, P, refs, src, note):
    px, pd = px.float().cpu().numpy().astype(np.float64), pd.float().cpu().numpy().astype(np.float64)
    assert (px[P:] == ROW_SENTINEL).all() and (pd[P:] == ROW_SENTINEL).all(), (note, "wrote past the last point")
    assert not px[:P, 63:].any() and not pd[:P, 27:].any(), (note, "pad columns")
    for entry, rows, n in (("l0", px, 63), ("posd", pd, 27)):
        for j in range(n):
            table.check(rows[:P, j:j + 1], refs, [(0, entry, j)], "bf16", src, note=note)


@pytest.mark.parametrize("lim", [4.5, 64.0, 4096.0])
def test_stored_rows_points(dev, probes, lim):
    """nerf_amd_encode_points_bf16 (csrc/encode.hip, sincos_rev_fast): all 63 + 27 stored columns against float64, pad
    columns exactly zero, rows >= P untouched."""
    L, lib = probes.L, probes.lib
    pts, refs, src = _sweep(lim)
    S = len(pts)
    table = Table(f"stored rows (points) lim={lim:g}", E=M.E_ROWS)
    for P in (S,) + (RAGGED_P if lim == 4.5 else ()):
        lo = 0 if P == S else (11 * P) % (S - P)
        v = torch.from_numpy(pts[lo:lo + P].copy()).to(dev).contiguous()
        px = torch.full((P + 8, 64), ROW_SENTINEL, dtype=torch.bfloat16, device=dev)
        pd = torch.full((P + 8, 32), ROW_SENTINEL, dtype=torch.bfloat16, device=dev)
        L.check(lib.nerf_amd_encode_points_bf16(L.ptr(v), L.ptr(px), L.ptr(pd), P, L.stream_ptr(dev)), "nerf_amd_encode_points_bf16")
        r, x = _slice(refs, src, lo, lo + P)
        _check_rows(table, px, pd, P, r, x, f"P={P}")
    table.finish()


def test_stored_rows_rays(dev, probes):
    """nerf_amd_sample_encode_bf16 on the ray shapes and on the value sweep, explicit positions."""
    L, lib = probes.L, probes.lib
    table = Table("stored rows (rays)", E=M.E_ROWS)
    for case in RAY_SHAPES + ("sweep",):
        B, N, rays_h, ts_h = _ray_case(case)
        rays = torch.from_numpy(rays_h).to(dev).contiguous()
        ts = torch.from_numpy(ts_h).to(dev).contiguous()
        refs, src = _refs(_query_points(probes, rays, ts, B, N).astype(np.float64))
        P = B * N
        px = torch.full((P + 8, 64), ROW_SENTINEL, dtype=torch.bfloat16, device=dev)
        pd = torch.full((P + 8, 32), ROW_SENTINEL, dtype=torch.bfloat16, device=dev)
        ts_out = torch.full((B, N), SENTINEL, device=dev)
        L.check(lib.nerf_amd_sample_encode_bf16(L.ptr(rays), L.ptr(ts), None, L.FLAG_TS_GIVEN, 0, 0, L.ptr(px), L.ptr(pd),
                                                L.ptr(ts_out), B, N, L.stream_ptr(dev)), "nerf_amd_sample_encode_bf16")
        assert torch.equal(ts_out, ts)
        _check_rows(table, px, pd, P, refs, src, f"{B}x{N}")
    table.finish()


# ---- beyond the accurate domain -------------------------------------------------------------------------------------------
HUGE = (1e6, 1e12, 1e30, float(np.finfo(np.float32).max))


def _huge_points(mag):
    """[12, 6]: +-mag in one column at a time, ordinary values elsewhere."""
    rows = []
    for c in range(6):
        for sgn in (1.0, -1.0):
            r = np.array([0.3, -0.7, 1.1, 0.6, -0.64, 0.48])
            r[c] = sgn * mag
            rows.append(r)
    return np.asarray(rows, dtype=np.float32)


@pytest.mark.parametrize("mag", HUGE, ids=lambda m: f"{m:.0e}")
def test_beyond_the_domain_stored_rows(dev, probes, mag):
    """|x| = 1e6 ... FLT_MAX through nerf_amd_encode_points_bf16: every sin / cos column finite with |f| <= 1 (nothing is said
    about the value: the reference's sinf(huge) is noise too); raw columns are round_bf16(x), which is inf at FLT_MAX."""
    L, lib = probes.L, probes.lib
    pts = _huge_points(mag)
    P = len(pts)
    v = torch.from_numpy(pts).to(dev).contiguous()
    px = torch.full((P, 64), ROW_SENTINEL, dtype=torch.bfloat16, device=dev)
    pd = torch.full((P, 32), ROW_SENTINEL, dtype=torch.bfloat16, device=dev)
    L.check(lib.nerf_amd_encode_points_bf16(L.ptr(v), L.ptr(px), L.ptr(pd), P, L.stream_ptr(dev)), "nerf_amd_encode_points_bf16")
    px, pd = px.float().cpu().numpy(), pd.float().cpu().numpy()
    print(f"|x| = {mag:.3e}: trig columns max |f| posx {np.nanmax(np.abs(px[:, 3:63])):.6f} posd {np.nanmax(np.abs(pd[:, 3:27])):.6f}, "
          f"non-finite {int((~np.isfinite(px[:, 3:63])).sum())} + {int((~np.isfinite(pd[:, 3:27])).sum())}")
    assert np.isfinite(px[:, 3:63]).all() and np.isfinite(pd[:, 3:27]).all()
    assert np.abs(px[:, 3:63]).max() <= 1.0 and np.abs(pd[:, 3:27]).max() <= 1.0
    with np.errstate(over="ignore"):
        assert np.array_equal(px[:, :3].astype(np.float64), M.round_to(pts[:, :3].astype(np.float64), "bf16"))
        assert np.array_equal(pd[:, :3].astype(np.float64), M.round_to(pts[:, 3:].astype(np.float64), "bf16"))


@pytest.mark.parametrize("mag", HUGE, ids=lambda m: f"{m:.0e}")
@pytest.mark.parametrize("path", ["fp16", "bf16"])
def test_beyond_the_domain_mlp(dev, probes, path, mag):
    """The same through nerf_amd_mlp_forward.  Where the raw coordinate fits the operand type (bf16 up to 1e30) every tapped
    trig feature is finite with |f| <= 1 and the non-finite status word stays clear.  Where it does not (fp16 beyond 65504,
    bf16 at FLT_MAX, which rounds to inf) the raw operand is inf and its products with the ZERO weights of every other unit
    are NaN: no tap can isolate a trig column there, and what is asserted is that the range guard reports it."""
    pts = _huge_points(mag)
    P = len(pts)
    v = torch.from_numpy(pts).to(dev).contiguous()
    T = OPERAND[path]
    with np.errstate(over="ignore"):
        fits = bool(np.isfinite(M.round_to(np.float64(mag), T)))
    flagged = 0
    worst = 0.0
    for s, taps in enumerate(probes.taps[False]):
        packed = probes.packed(s, path)
        got = _forward_points(probes, path, packed, v, P)[:P].cpu().numpy()
        status = probes.status(packed, path)
        probes.clear_status(packed, path)                     # the images are shared with the other tests
        if fits:
            assert status == (0, 0), (path, mag, s)
            for ch, entry, col in taps:
                if col >= 3:
                    assert np.isfinite(got[:, ch]).all() and np.abs(got[:, ch]).max() <= 1.0, (path, mag, entry, col, got[:, ch])
                    worst = max(worst, float(np.abs(got[:, ch]).max()))
        else:
            flagged += status[0]
    print(f"{path} |x| = {mag:.3e}: operand {'fits' if fits else 'overflows'}, max |trig feature| {worst:.6f}, "
          f"weight sets flagged non-finite {flagged} of {len(probes.taps[False])}")
    if not fits:
        assert flagged == len(probes.taps[False])


# ---- the fused render composes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["bf16", "fp16", "fp32"])
def test_fused_render_composes_on_probe_weights(dev, probes, path):
    """nerf_amd_render_forward (COMP instantiation: samples composited out of the LDS ring) against nerf_amd_mlp_forward_rays
    + nerf_amd_volume_render_rays on the same rays, positions and probe weights -- one weight set per entry point -- bit for
    bit, as test_fused_render_equals_two_launch_path asserts it for that precision.  With the rays-path tests above this
    pins the encoder of the fused render."""
    L, lib = probes.L, probes.lib
    code = probes.code(path)
    st = L.stream_ptr(dev)
    chosen = [next(s for s, taps in enumerate(probes.taps[False]) if any(e == entry for _, e, _ in taps))
              for entry in ("l0", "skip", "posd")]
    for B, N in RAY_SHAPES[1:]:
        rays_h, ts_h = M.probe_rays(B, N)
        rays = torch.from_numpy(rays_h).to(dev).contiguous()
        ts = torch.from_numpy(ts_h).to(dev).contiguous()
        assert lib.nerf_amd_render_workspace_bytes(code, B, N) == 0
        for s in chosen:
            packed = probes.packed(s, path)
            raw, ts_out = _forward_rays(probes, path, packed, rays, ts, B, N, pad=0)
            two = [torch.full(s_, 7.0, device=dev) for s_ in ((B, 3), (B,), (B, N), (B,), (B, N))]
            L.check(lib.nerf_amd_volume_render_rays(L.ptr(raw), L.ptr(ts_out), L.ptr(rays), *[L.ptr(x) for x in two], B, N, st),
                    "nerf_amd_volume_render_rays")
            one = [torch.full(s_, -7.0, device=dev) for s_ in ((B, 3), (B,), (B, N), (B,), (B, N))]
            L.check(lib.nerf_amd_render_forward(L.ptr(rays), L.ptr(ts), None, L.ptr(packed), code, L.FLAG_TS_GIVEN, 0, 0,
                                                *[L.ptr(x) for x in one], None, B, N, st), "nerf_amd_render_forward")
            torch.cuda.synchronize()
            assert raw.abs().max() > 0 and torch.isfinite(two[0]).all()
            for name, a, b in zip(("rgb", "disp", "alpha", "acc", "w"), one, two):
                assert torch.equal(a, b), (path, B, N, s, name, float((a - b).abs().max()))
