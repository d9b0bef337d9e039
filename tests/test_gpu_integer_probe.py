"""GPU tests that pin the inference network kernels on exact-integer probe weights (tests/integer_probe_model.py; DESIGN.md
"Integer probe").

Every weight, bias and activation of a probe set is a small multiple of 1/4, exactly representable in the kernel's operand
type, and no dot product can pass 2^24 quanta: whatever the summation order, a correct kernel returns the float64 forward
bit for bit.  Every assertion here is an equality with the model's float64 output cast to fp32: no tolerance, no factor, no
point and no output left out.

  points mode   nerf_amd_mlp_forward fp32 / bf16 / fp16, every set, P = 1, 255, 257 and P_big = 2 T CUs + 300 (T = 256
                points per tile, 128 in fp32: every workgroup runs two tiles at least, some three, the last one partial);
  module        Nerf.forward in the three precisions, the fp16 / bf16 status words clear, no warning of the range guard;
  density       Nerf.density (the sigma-only plan of csrc/density.hip) fp16 / bf16, rows of three and of six floats;
  rays mode     nerf_amd_mlp_forward_rays with the probe rays, bins and jitter, N = 4 and 8, B N >= P_big and a ragged B;
  fused render  nerf_amd_render_forward / nerf_amd_render_pixels_forward == nerf_amd_volume_render_rays / _pixels applied
                to the exact raw: the one-launch kernel's chain is pinned through the pinned raw;
  generic path  Nerf(2, 1, 64) on csrc/linear_generic.hip: forward and every parameter gradient on integer weights.
"""
import warnings

import numpy as np
import pytest
import torch

import integer_probe_model as M

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
PRECISIONS = ("fp32", "bf16", "fp16")
TILE = {"fp32": 128, "bf16": 256, "fp16": 256}
SMALL_P = (1, 255, 257)
RAGGED_B = 37


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with a GPU: pytest -m gpu"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


class Probes:
    """The probe sets on the device; packed images on first use per precision."""

    def __init__(self, dev, synthetic):
        from nerf_simple_amd import _lib
        self.dev, self.L, self.lib, self.synthetic = dev, _lib, _lib.lib(), synthetic
        self.sets = M.probe_sets()
        self.images = {}
        self.cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def p_big(self, T):
        return 2 * TILE[T] * self.cus + 300

    def packed(self, ps, T):
        key = (ps.index, T)
        if key not in self.images:
            code = self.L.precision_code(T)
            flat = self.synthetic.flatten_state_dict(ps.sd).to(self.dev)
            buf = torch.empty(self.lib.nerf_amd_packed_bytes(code), dtype=torch.uint8, device=self.dev)
            self.L.check(self.lib.nerf_amd_pack_weights(self.L.ptr(flat), self.L.ptr(buf), code, self.L.stream_ptr(self.dev)),
                         "nerf_amd_pack_weights")
            self.images[key] = buf
        return self.images[key]

    def status(self, ps, T):
        off = int(self.lib.nerf_amd_packed_status_offset(self.L.precision_code(T)))
        return tuple(int(x) for x in self.packed(ps, T)[off:off + 8].view(torch.int32).cpu())


@pytest.fixture(scope="module")
def probes(dev, synthetic):
    return Probes(dev, synthetic)


class Diffs:
    """Collects unequal comparisons; `finish` fails with the count and the first differing (set, point, output) of each."""

    def __init__(self):
        self.lines, self.compared = [], 0

    def equal(self, got, want, what):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
        self.compared += got.size
        same = (got == want) | (np.isnan(got) & np.isnan(want))
        if not same.all():
            first = tuple(int(i) for i in np.argwhere(~same)[0])
            self.lines.append(f"{what}: {int((~same).sum())} of {got.size} differ, first at {first}: got {got[first]!r} want {want[first]!r}")

    def finish(self):
        print(f"{self.compared} values compared for equality")
        assert not self.lines, f"{len(self.lines)} unequal comparisons\n" + "\n".join(self.lines[:16])


def _points(ps, P):
    """(v [P, 6] fp32, the model's outputs [P, 4] fp32): the set's base batch, tiled."""
    u = M.universe(ps.zero)
    i = np.arange(P) % M.BASE_POINTS
    return M.probe_points(ps.zero)[i], ps.out[u.points[i]].astype(np.float32)


def _rays(ps, B, N):
    """(rays [B, 6], tb [N + 1], u [B, N], ts [B, N], raw [B N, 4]) fp32: the set's base rays, tiled, and the model's ts and raw."""
    uni = M.universe(ps.zero)
    rays, tb, u = M.probe_rays(N, ps.zero)
    i = np.arange(B) % M.BASE_RAYS
    rows = uni.rays[N].reshape(M.BASE_RAYS, N)[i].reshape(-1)
    ts = uni.ts[N][i]
    assert np.array_equal(ts.astype(np.float32).astype(np.float64), ts)
    return rays[i], tb, u[i], ts.astype(np.float32), ps.out[rows].astype(np.float32)


def _dev(probes, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(probes.dev) for a in arrays]


# ---- points mode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", PRECISIONS)
def test_points_mode(dev, probes, T):
    """nerf_amd_mlp_forward on every set of the precision, into a sentinel-padded buffer: rows below P equal the float64
    forward, rows from P on are untouched."""
    L, lib = probes.L, probes.lib
    code = L.precision_code(T)
    diffs = Diffs()
    for ps in M.sets_for(T):
        packed = probes.packed(ps, T)
        for P in SMALL_P + (probes.p_big(T),):
            v_h, want = _points(ps, P)
            v, = _dev(probes, v_h)
            out = torch.full((P + 64, 4), SENTINEL, device=dev)
            L.check(lib.nerf_amd_mlp_forward(L.ptr(v), L.ptr(packed), L.ptr(out), P, code, L.stream_ptr(dev)), "nerf_amd_mlp_forward")
            host = out.cpu().numpy()
            assert (host[P:] == SENTINEL).all(), (T, ps, P, "wrote past the last point")
            diffs.equal(host[:P], want, f"{T} {ps.name} P={P}")
        if T != "fp32":
            assert probes.status(ps, T) == (0, 0), (T, ps)
    diffs.finish()


# ---- the module --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", PRECISIONS)
def test_module_forward_and_status(dev, probes, T):
    """Nerf.forward gives the same values, the range guard sees nothing (status words clear, no demotion warning)."""
    from nerf_simple_amd.utils.nets import Nerf, packed_status
    net = Nerf(precision=T).to(dev)
    diffs = Diffs()
    P = M.BASE_POINTS + 7
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for ps in M.sets_for(T):
            net.load_state_dict(ps.sd)
            v_h, want = _points(ps, P)
            v, = _dev(probes, v_h)
            with torch.no_grad():
                got = net(v)
            diffs.equal(got.cpu().numpy(), want, f"Nerf.forward {T} {ps.name}")
            if T != "fp32":
                assert packed_status(net.packed_weights(), probes.L.precision_code(T)) == 0, (T, ps)
    guard = [str(w.message) for w in caught if str(w.message).startswith("Nerf:")]
    assert not guard, guard
    diffs.finish()


@pytest.mark.parametrize("T", ["fp16", "bf16"])
def test_density(dev, probes, T):
    """Nerf.density (the sigma-only kernel) equals the model's sigma, rows of three and of six floats."""
    from nerf_simple_amd.utils.nets import Nerf
    net = Nerf(precision=T).to(dev)
    diffs = Diffs()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for ps in M.sets_for(T):
            net.load_state_dict(ps.sd)
            for P, width in ((257, 3), (M.BASE_POINTS + 7, 6), (2 * 256 + 3, 3)):
                v_h, want = _points(ps, P)
                x, = _dev(probes, v_h[:, :width])
                with torch.no_grad():
                    got = net.density(x)
                diffs.equal(got.cpu().numpy(), want[:, 3], f"density {T} {ps.name} P={P} width {width}")
    guard = [str(w.message) for w in caught if str(w.message).startswith("Nerf:")]
    assert not guard, guard
    diffs.finish()


# ---- rays mode and the fused render --------------------------------------------------------------------------------------------
def _ray_batches(probes, T):
    return [(B, N) for N in M.RAY_N for B in (RAGGED_B, -(-probes.p_big(T) // N))]


@pytest.mark.parametrize("T", PRECISIONS)
def test_rays_mode(dev, probes, T):
    """nerf_amd_mlp_forward_rays samples, encodes and runs the chain: the returned ts and raw equal the model's."""
    L, lib = probes.L, probes.lib
    code = L.precision_code(T)
    diffs = Diffs()
    for ps in M.sets_for(T):
        packed = probes.packed(ps, T)
        for B, N in _ray_batches(probes, T):
            rays_h, tb_h, u_h, ts_want, raw_want = _rays(ps, B, N)
            rays, tb, u = _dev(probes, rays_h, tb_h, u_h)
            raw = torch.full((B * N + 16, 4), SENTINEL, device=dev)
            ts = torch.full((B, N), SENTINEL, device=dev)
            L.check(lib.nerf_amd_mlp_forward_rays(L.ptr(rays), L.ptr(u), L.ptr(tb), L.ptr(packed), code, 0, 0, 0, L.ptr(raw),
                                                  L.ptr(ts), B, N, L.stream_ptr(dev)), "nerf_amd_mlp_forward_rays")
            host = raw.cpu().numpy()
            assert (host[B * N:] == SENTINEL).all(), (T, ps, B, N, "wrote past the last sample")
            diffs.equal(ts.cpu().numpy(), ts_want, f"ts {T} {ps.name} {B}x{N}")
            diffs.equal(host[:B * N], raw_want, f"raw {T} {ps.name} {B}x{N}")
        if T != "fp32":
            assert probes.status(ps, T) == (0, 0), (T, ps)
    diffs.finish()


@pytest.mark.parametrize("T", PRECISIONS)
def test_fused_render(dev, probes, T):
    """nerf_amd_render_forward and nerf_amd_render_pixels_forward on the probe rays against the compositor kernels applied to
    the exact raw and ts of the model (which test_rays_mode holds the rays-mode kernel to): bit for bit."""
    L, lib = probes.L, probes.lib
    code = L.precision_code(T)
    st = L.stream_ptr(dev)
    diffs = Diffs()
    opaque = batches = 0
    for ps in M.sets_for(T):
        packed = probes.packed(ps, T)
        for B, N in _ray_batches(probes, T):
            rays_h, tb_h, u_h, ts_want, raw_want = _rays(ps, B, N)
            rays, tb, u, ts, raw = _dev(probes, rays_h, tb_h, u_h, ts_want, raw_want)
            shapes = ((B, 3), (B,), (B, N), (B,), (B, N))
            two = [torch.full(s, 7.0, device=dev) for s in shapes]
            L.check(lib.nerf_amd_volume_render_rays(L.ptr(raw), L.ptr(ts), L.ptr(rays), *[L.ptr(x) for x in two], B, N, st),
                    "nerf_amd_volume_render_rays")
            two_px = torch.full((B, 4), 7.0, device=dev)
            L.check(lib.nerf_amd_volume_render_pixels(L.ptr(raw), L.ptr(ts), L.ptr(rays), L.ptr(two_px), B, N, st),
                    "nerf_amd_volume_render_pixels")
            nws = int(lib.nerf_amd_render_workspace_bytes(code, B, N))
            ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
            one = [torch.full(s, -7.0, device=dev) for s in shapes]
            L.check(lib.nerf_amd_render_forward(L.ptr(rays), L.ptr(u), L.ptr(tb), L.ptr(packed), code, 0, 0, 0,
                                                *[L.ptr(x) for x in one], L.ptr(ws), B, N, st), "nerf_amd_render_forward")
            one_px = torch.full((B, 4), -7.0, device=dev)
            L.check(lib.nerf_amd_render_pixels_forward(L.ptr(rays), L.ptr(u), L.ptr(tb), L.ptr(packed), code, 0, 0, 0,
                                                       L.ptr(one_px), L.ptr(ws), B, N, st), "nerf_amd_render_pixels_forward")
            for name, a, b in zip(("rgb", "disp", "alpha", "acc", "w"), one, two):
                diffs.equal(a.cpu().numpy(), b.cpu().numpy(), f"render {name} {T} {ps.name} {B}x{N}")
            diffs.equal(one_px.cpu().numpy(), two_px.cpu().numpy(), f"render pixels {T} {ps.name} {B}x{N}")
            assert np.isfinite(two[0].cpu().numpy()).all(), (T, ps, B, N)
            opaque += int(float(two[3].max()) > 0)
            batches += 1
    print(f"{T}: {opaque} of {batches} (set, batch) renders have a ray with acc > 0")
    assert 2 * opaque >= batches                   # sanity: the comparison is not one of empty images throughout
    diffs.finish()


# ---- the layer-by-layer path ---------------------------------------------------------------------------------------------------
SMALL = (2, 1, 64)


def _forward_keeping(oracle, sd, v, Lp, Ld):
    """The reference forward (oracle.nerf_forward's data flow) in the dtype of sd, keeping the outputs of the three encoder-fed
    layers before their ReLU, so that their gradients dy can be read after backward."""
    import torch.nn.functional as F
    lin = lambda h, name: F.linear(h, sd[name + ".weight"], sd[name + ".bias"])       # noqa: E731
    x, d = oracle.positional_encoder(v, Lp, Ld)
    z = {"layers_0.0": lin(x, "layers_0.0")}
    h = F.relu(z["layers_0.0"])
    for i in (2, 4, 6, 8):
        h = F.relu(lin(h, f"layers_0.{i}"))
    z["skip_conn_layer.0"] = lin(torch.cat([h, x], 1), "skip_conn_layer.0")
    h = F.relu(z["skip_conn_layer.0"])
    for i in (0, 2):
        h = F.relu(lin(h, f"layers_1.{i}"))
    z["color_fc.0"] = lin(torch.cat([lin(h, "layers_2"), d], 1), "color_fc.0")
    rgb = lin(F.relu(z["color_fc.0"]), "color_fc.2")
    for t in z.values():
        t.retain_grad()
    return torch.cat([rgb, lin(h, "sigma_fc.0")], 1), z


@pytest.mark.parametrize("P", [257, 20000])
@pytest.mark.parametrize("dense", ["layers_0.4", "skip_conn_layer.0", "color_fc.0"])
def test_generic_path_on_integers(dev, oracle, dense, P):
    """Nerf(2, 1, 64) runs layer by layer in fp32 (csrc/linear_generic.hip).  On integer weights and points the forward
    equals the float64 forward, and with an integer g_out every parameter gradient whose terms are integers equals the
    float64 gradient: every partial sum is an integer below 2^24 (asserted on sum |terms|), so the split-K atomics and
    the column sums are exact in any order.  The only other entries are the trig columns of the three encoder-fed weights:
    their terms dy sin(2^l x) are no integers.  They are held to what fp32 allows: (sum_p |dy[p, row]|) (ENC_ATOL + P 2^-24),
    the feature's error (encoder_probe_model.ENC_ATOL, the exact encoder's bound) plus the worst case of rounding P fp32
    products and additions of terms |dy f| <= |dy|; dy is the float64 reference's own (an integer)."""
    from encoder_probe_model import ENC_ATOL
    from nerf_simple_amd.utils.nets import Nerf
    Lp, Ld, H = SMALL
    sd = M.small_state_dict(Lp, Ld, H, dense, seed=P % 2)
    rng = np.random.Generator(np.random.PCG64(P))
    # x in [-2, 2]^3, d in {-1, 0, 1}^3; g_out in {-1, 0, 1}, zero at half of the points: sum |terms| stays below 2^24 at P = 20000
    v64 = torch.from_numpy(np.concatenate([rng.integers(-2, 3, (P, 3)), rng.integers(-1, 2, (P, 3))], 1).astype(np.float64))
    g64 = torch.from_numpy((rng.integers(-1, 2, (P, 4)) * rng.integers(0, 2, (P, 1))).astype(np.float64))
    ref = {k: t.double().requires_grad_(True) for k, t in sd.items()}
    want, z = _forward_keeping(oracle, ref, v64, Lp, Ld)
    want.backward(g64)
    assert torch.equal(want, oracle.nerf_forward({k: t.detach() for k, t in ref.items()}, v64, Lp, Ld))
    net = Nerf(Lp, Ld, H).to(dev)
    net.load_state_dict(sd)
    out = net(v64.float().to(dev))
    out.backward(g64.float().to(dev))
    diffs = Diffs()
    assert want.abs().max() < 2 ** 24 and (want == want.round()).all() and want.std(0).min() > 0
    diffs.equal(out.detach().cpu().numpy(), want.detach().numpy().astype(np.float32), f"forward {dense} P={P}")
    # sum |terms| of every gradient entry: the same backward with |g_out| through |W|, every ReLU taken as open
    absref = {k: t.detach().abs().requires_grad_(True) for k, t in ref.items()}
    big = oracle.nerf_forward(absref, v64.abs(), Lp, Ld)
    big.backward(g64.abs())
    worst = 0.0
    for k, p in net.named_parameters():
        g, exact = ref[k].grad.detach().numpy(), np.ones(ref[k].shape, bool)
        for name, base, levels in (("layers_0.0.weight", 0, Lp), ("skip_conn_layer.0.weight", H, Lp), ("color_fc.0.weight", H, Ld)):
            if k == name:
                exact[:, base + 3:base + 3 + 6 * levels] = False
        bound = absref[k].grad.numpy()[exact].max(initial=0.0)
        worst = max(worst, float(bound))
        assert bound < 2 ** 24, (k, bound)
        assert (g[exact] == np.rint(g[exact])).all() and np.abs(g[exact]).max() > 0, k
        got = p.grad.cpu().numpy()
        diffs.equal(got[exact], g[exact].astype(np.float32), f"grad {k} {dense} P={P}")
        if not exact.all():
            dy_abs = z[k[:-7]].grad.abs().sum(0).numpy()[:, None]          # sum_p |dy[p, row]|
            err = np.abs(got.astype(np.float64) - g)[~exact]
            allow = np.broadcast_to(dy_abs * (ENC_ATOL + P * 2.0 ** -24), g.shape)[~exact]
            print(f"{k} trig columns: max |err| / allowance {np.max(err / np.maximum(allow, 1e-300)):.3f}, max |err| {err.max():.3e}")
            assert (err <= allow).all(), (k, float((err - allow).max()))
    print(f"{dense} P={P}: largest sum |terms| of an exact gradient entry {worst:.0f} (< 2^24 = {2 ** 24})")
    diffs.finish()
