"""Early ray termination on the GPU (csrc/occupancy_terminate.hip, utils/occupancy.py EarlyTermination).

Kernel level: nerf_amd_termination_advance is driven slab by slab through the C ABI on rows the test chooses (no network runs).
What it selects must be, bit for bit, M0 & range & !(trans < eps) of its OWN trans; what it retires must be bit-equal to its
source; its trans must agree with the float64 product of the factors (alpha from nerf_amd_volume_render_masked on the same rows)
within 2 N 2^-24 relative (N rounded factors and N rounded multiplies) plus N 1e-10 (the 1e-10 fp32 drops from a factor), and
outside that band around eps its liveness must be the model's (tests/termination_model.py).

Render level: render_nerf / render_view(..., terminate=) must equal, bit for bit, nerf_amd_query_points -> nerf_amd_mlp_forward on
all B N points -> rows outside EarlyTermination.evaluated_mask overwritten with (0, 0, 0, -inf) -> nerf_amd_volume_render_rays.

Inputs: camera spherical_to_pose(4, -30, 40), t in [2, 6], torch.manual_seed(0) jitter; 20 x 20 rays where a share is asserted
(tests/test_termination_cpu.py recomputes those shares on the CPU oracle), 32 x 32 where 1000 rays are needed; the radius-1 ball
in a 129^3 grid over [-1.5, 1.5]^3."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import occupancy_model as M
import termination_model as T

pytestmark = pytest.mark.gpu

NAMES = ("rgb", "disp", "alpha", "acc", "w")
SENTINEL = 0x5A
PAD = 64                                     # sentinel bytes are checked behind every buffer the kernel writes


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def make_net(dev, kind, precision=None, sd=None):
    from nerf_simple_amd.utils import synthetic
    from nerf_simple_amd.utils.nets import Nerf
    net = Nerf(precision=precision).to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, kind) if sd is None else sd)
    return net


_scene = {}


def grid(dev, which):
    """'ball-empty' / 'ball-live' (the radius-1 ball, either outside policy), 'all' (an explicit all-live grid), 'dead'"""
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    if which not in _scene:
        if which.startswith("ball"):
            if "ball" not in _scene:
                _scene["ball"] = M.ball_cells(T.R129, T.BOUNDS, 1.0)
            _scene[which] = OccupancyGrid.from_mask(torch.from_numpy(_scene["ball"]).to(dev), T.BOUNDS, outside=which[5:])
        elif which == "all":
            _scene[which] = OccupancyGrid.from_mask(torch.ones(4, 4, 4, dtype=torch.bool, device=dev), T.BOUNDS, outside="live")
        else:
            _scene[which] = OccupancyGrid.from_mask(torch.zeros(4, 4, 4, dtype=torch.bool, device=dev), T.BOUNDS, outside="empty")
    return _scene[which]


def subset(n, B):
    return np.array([n // 2 + int(n ** 0.5) // 2]) if B == 1 else np.linspace(0, n - 1, B).astype(np.int64)


def tbins(N, dev):
    from nerf_simple_amd.utils.rendering import _tbins
    return _tbins(2, 6, N, dev)


def unpack(mask, N):
    """int64 [B, W] device mask words -> bool [B, N] numpy"""
    w = mask.cpu().numpy().view(np.uint64)
    b = (w[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return b.reshape(w.shape[0], -1)[:, :N].astype(bool)


def padded(shape_elems, dtype, dev):
    """a flat buffer of shape_elems elements followed by PAD sentinel bytes; returns (whole byte buffer, typed view)"""
    nbytes = shape_elems * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((nbytes + PAD,), SENTINEL, dtype=torch.uint8, device=dev)
    return buf, buf[:nbytes].view(dtype)


def tail_ok(buf):
    return bool((buf[-PAD:] == SENTINEL).all())


# ---- 1. the kernel, slab by slab through the C ABI --------------------------------------------------------------------------
def drive(dev, lib, head, m, raw_live, eps, S, B, N):
    """All K + 1 calls of nerf_amd_termination_advance on the rows raw_live [P'0, 4] (M0 layout).  Every call's selection is
    checked against the kernel's own trans.  Returns (raw0, trans [B, K], evaluated bool [B, N], sentinels intact, every buffer's
    bytes)."""
    from nerf_simple_amd import _lib
    K, W = T.slab_count(N, S), (N + 63) // 64
    live0 = unpack(m.mask, N)
    off0 = m.offsets.cpu().numpy()
    row0 = off0[:-1, None] + np.cumsum(live0, 1) - 1                     # the M0 row of a live sample
    raw0_buf, raw0 = padded(max(m.live, 1) * 4, torch.float32, dev)
    raw0 = raw0.view(-1, 4)
    raw0[:] = torch.tensor([0.0, 0.0, 0.0, -np.inf], device=dev)
    trans_buf, trans = padded(B * K, torch.float32, dev)
    trans = trans.view(B, K)
    mbuf, masks, obuf, offs = [], [], [], []
    for _ in range(2):
        b, v = padded(B * W, torch.int64, dev)
        mbuf.append(b), masks.append(v.view(B, W))
        b, v = padded(B + 1, torch.int64, dev)
        obuf.append(b), offs.append(v)
    tot_buf, totals = padded(2, torch.int64, dev)
    ws_bytes = int(lib.nerf_amd_termination_workspace_bytes(B))
    ws_buf = torch.full((ws_bytes + PAD,), SENTINEL, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    evaluated = np.zeros((B, N), dtype=bool)
    cur, raw_slab, rows = 1, None, 0
    for s0, s1, s2 in T.advance_calls(N, S):
        rc = lib.nerf_amd_termination_advance(
            _lib.ptr(raw_slab), _lib.ptr(masks[cur]) if raw_slab is not None else None,
            _lib.ptr(offs[cur]) if raw_slab is not None else None, rows, *head, _lib.ptr(m.mask), _lib.ptr(m.offsets), _lib.ptr(raw0),
            m.live, ctypes.c_float(eps), S, s0, s1, s2, _lib.ptr(trans), _lib.ptr(masks[1 - cur]), _lib.ptr(offs[1 - cur]),
            _lib.ptr(totals), _lib.ptr(ws_buf), B, N, st)
        assert rc == 0, (rc, s0, s1, s2)
        cur = 1 - cur
        sel = unpack(masks[cur], N)
        rng_ = np.zeros(N, dtype=bool)
        rng_[s1:s2] = True
        if s1 < N:
            tk = trans[:, s1 // S].cpu().numpy()
            with np.errstate(invalid="ignore"):
                alive = ~(tk < np.float32(eps))
        else:
            alive = np.zeros(B, dtype=bool)
        want = live0 & rng_[None, :] & alive[:, None]
        assert (sel == want).all(), ("mask_next", s0, s1, s2)
        assert (masks[cur].cpu().numpy().view(np.uint64) == M.mask_words(want)).all(), ("mask_next words", s1)      # bits >= N zero
        assert (offs[cur].cpu().numpy() == M.offsets(want)).all(), ("offsets_next", s1)
        beyond = np.zeros(N, dtype=bool)
        beyond[s1:] = True
        assert totals.tolist() == [int(want.sum()), int((live0 & beyond[None, :] & alive[:, None]).sum())], ("totals", s1)
        # the next slab's rows, compacted in the order of nerf_amd_occupancy_points
        rows = int(want.sum())
        raw_slab = raw_live[torch.from_numpy(row0[want]).to(dev)].contiguous() if rows else None
        evaluated |= want
    intact = all(tail_ok(b) for b in (raw0_buf, trans_buf, tot_buf, ws_buf, *mbuf, *obuf))
    everything = [b.clone() for b in (raw0_buf, trans_buf, tot_buf, *mbuf, *obuf)]
    return raw0, trans, evaluated, live0, row0, intact, everything


@pytest.mark.parametrize("outside", ["empty", "live"])
@pytest.mark.parametrize("mode", ["u", "ts", "device_rng"])
def test_advance_kernel_against_its_own_trans_and_the_float64_model(dev, oracle, synthetic, mode, outside):
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils.occupancy import sample_positions
    lib = _lib.lib()
    occ = grid(dev, "ball-" + outside)
    gen = torch.Generator().manual_seed(20 + ("u", "ts", "device_rng").index(mode) * 2 + (outside == "live"))
    dead_bits = bits(torch.tensor([0.0, 0.0, 0.0, -np.inf]))
    terminated_somewhere = dropped_somewhere = nan_seen = 0
    for N in (3, 33, 64, 65, 128, 192, 768):
        _, rays_all, u_all, _, _, _ = T.view(oracle, synthetic, N)
        for B in (1, 37, 300):
            idx = subset(rays_all.shape[0], B)
            rays = rays_all[idx].contiguous().to(dev)
            u = u_all[idx].contiguous().to(dev)
            tb = tbins(N, dev)
            if mode == "u":
                jit, flags, seed, ray_id0, kw = u, 0, 0, 0, dict(u=u)
            elif mode == "ts":
                ts = sample_positions(rays, u, tb, 0, 0, 0, N)
                jit, flags, seed, ray_id0, tb, kw = ts, _lib.FLAG_TS_GIVEN, 0, 0, None, dict(ts=ts)
            else:
                jit, flags, seed, ray_id0, kw = None, _lib.FLAG_DEVICE_RNG, 11, 5, dict(device_rng=True, seed=11, ray_id0=5)
            m = occ.mark(rays, N, **kw)
            head = (_lib.ptr(rays), _lib.ptr(jit), _lib.ptr(tb), flags, seed, ray_id0)
            P0 = m.live
            live_per_ray = (m.offsets[1:] - m.offsets[:-1]).cpu().numpy()
            for kind in ("random", "opaque"):
                raw_live = torch.rand(max(P0, 1), 4, generator=gen)
                if kind == "random":
                    # densities around the point where T crosses eps inside the ray: delta ~ 4 / N
                    raw_live[:, 3] = torch.randn(max(P0, 1), generator=gen) * 2.0 + np.log(np.expm1(min(N / 48.0, 30.0)))
                    eps = 0.5
                else:
                    raw_live[:, 3] = torch.where(torch.rand(max(P0, 1), generator=gen) < 0.3, 30.0, -30.0)
                    eps = 1e-3
                nan_ray = B - 1 if live_per_ray[B - 1] > 0 else int(np.argmax(live_per_ray > 0))
                if P0:
                    raw_live[int(m.offsets[nan_ray])] = torch.tensor([0.5, float("nan"), 0.5, float("nan")])   # its first live sample
                raw_live = raw_live.to(dev)
                # alpha of every M0 sample, from the masked compositor on the same rows
                outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in ((B, 3), (B,), (B, N), (B,), (B, N))]
                _lib.check(lib.nerf_amd_volume_render_masked(_lib.ptr(raw_live), *head, _lib.ptr(m.mask), _lib.ptr(m.offsets),
                                                             *[_lib.ptr(o) for o in outs], B, N, _lib.stream_ptr(dev)), "masked")
                alpha = outs[2].cpu().numpy().astype(np.float64)
                for S in T.SLABS:
                    case = (mode, outside, N, B, kind, S)
                    K = T.slab_count(N, S)
                    raw0, trans, evaluated, live0, row0, intact, everything = drive(dev, lib, head, m, raw_live, eps, S, B, N)
                    assert intact, case
                    # retired rows are bit-equal to their source, unwritten rows still (0, 0, 0, -inf)
                    if P0:
                        wrote = np.zeros(P0, dtype=bool)
                        wrote[row0[evaluated]] = True
                        wrote = torch.from_numpy(wrote).to(dev)
                        assert torch.equal(bits(raw0)[wrote], bits(raw_live)[wrote]), case
                        assert (bits(raw0)[~wrote] == dead_bits.to(dev)).all(), case
                    # trans against float64, liveness against the model, outside the band around eps
                    T64, ev64, term64 = T.terminate(alpha, live0, S, eps, exact_factor=True)
                    got = trans.cpu().numpy().astype(np.float64)
                    tol = 2 * N * 2.0 ** -24 * np.abs(T64) + N * 1e-10
                    with np.errstate(invalid="ignore"):
                        in_band = (np.abs(T64 - eps) <= tol).any(1)
                        gpu_term = got < eps
                    assert in_band.mean() <= 0.01, (case, "the float64 model itself leaves more than 1 % of the rays in the band")
                    keep = ~in_band
                    assert (gpu_term[keep] == term64[keep]).all(), case
                    assert (evaluated[keep] == ev64[keep]).all(), case
                    nan64 = np.isnan(T64)
                    assert (np.isnan(got)[keep] == nan64[keep]).all(), case
                    ok = keep[:, None] & ~nan64
                    assert (np.abs(got - T64)[ok] <= tol[ok]).all(), (case, float(np.nanmax(np.abs(got - T64)[ok] / tol[ok])))
                    assert (got[:, 0] == 1).all(), case
                    if P0 and live_per_ray[nan_ray] > 0 and int(np.argmax(live0[nan_ray])) < (K - 1) * S:
                        # the NaN row: T is NaN from the next slab on and the ray is never terminated
                        first = int(np.argmax(live0[nan_ray])) // S
                        assert np.isnan(got[nan_ray, first + 1:]).all() and (evaluated[nan_ray] == live0[nan_ray]).all(), case
                        nan_seen += 1
                    terminated_somewhere += int(gpu_term.any())
                    dropped_somewhere += int(evaluated.sum() < live0.sum())
                    if S == 32:                                     # two runs write the same bytes
                        again = drive(dev, lib, head, m, raw_live, eps, S, B, N)[-1]
                        assert all(torch.equal(a, b) for a, b in zip(everything, again)), case
    assert terminated_somewhere > 20 and dropped_somewhere > 20 and nan_seen > 10


# ---- 2. the render against the composition of entry points that existed before it ------------------------------------------
def composed(dev, net, code, rays, jit, tb, flags, seed, ray_id0, N, evaluated_mask, pixels=False):
    """query points -> the network on all B N points -> rows outside evaluated_mask overwritten -> the dense compositor; also
    returns the network's rows [B, N, 4] before the overwrite"""
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils.rendering import _query_points
    lib = _lib.lib()
    B = rays.shape[0]
    q, ts = _query_points(rays, jit, tb, flags, seed, ray_id0, N)
    raw = torch.empty((B * N, 4), dtype=torch.float32, device=dev)
    st = _lib.stream_ptr(dev)
    _lib.check(lib.nerf_amd_mlp_forward(_lib.ptr(q), _lib.ptr(net.packed_weights(code)), _lib.ptr(raw), B * N, code, st), "forward")
    full = raw.clone().view(B, N, 4)
    shifts = torch.arange(64, dtype=torch.int64, device=dev)
    ev = ((evaluated_mask[:, :, None] >> shifts) & 1).reshape(B, -1)[:, :N].bool()
    raw[~ev.reshape(-1)] = torch.tensor([0.0, 0.0, 0.0, -np.inf], device=dev)
    if pixels:
        px = torch.empty((B, 4), dtype=torch.float32, device=dev)
        _lib.check(lib.nerf_amd_volume_render_pixels(_lib.ptr(raw), _lib.ptr(ts), _lib.ptr(rays), _lib.ptr(px), B, N, st), "pixels")
        return px, full, ev
    outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in ((B, 3), (B,), (B, N), (B,), (B, N))]
    _lib.check(lib.nerf_amd_volume_render_rays(_lib.ptr(raw), _lib.ptr(ts), _lib.ptr(rays), *[_lib.ptr(o) for o in outs], B, N, st),
               "composite")
    return tuple(outs), full, ev


@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_terminated_render_equals_the_composition_bit_for_bit(dev, oracle, synthetic, precision, kind):
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils.occupancy import EarlyTermination
    from nerf_simple_amd.utils.rendering import render_nerf
    net = make_net(dev, kind, precision)
    code = _lib.precision_code(precision)
    eps = 0.1 if kind == "structured" else 0.9          # (the fog of the default weights terminates nothing at 0.1)
    dropped = 0
    for n, N in enumerate((64, 65, 128, 192)):
        _, rays_all, u_all, _, _, _ = T.view(oracle, synthetic, N, n_side=32)
        for b, B in enumerate((1, 63, 1000)):
            idx = subset(rays_all.shape[0], B)
            rays, u, tb = rays_all[idx].contiguous().to(dev), u_all[idx].contiguous().to(dev), tbins(N, dev)
            for g, which in enumerate((None, "ball-empty")):
                term = EarlyTermination(eps if which is None else 0.5, T.SLABS[(n + b + g) % 3])
                occ = None if which is None else grid(dev, which)
                with torch.no_grad():
                    got = render_nerf(rays, net, N, u=u, occupancy=occ, terminate=term)
                (want, _, ev) = composed(dev, net, code, rays, u, tb, 0, 0, 0, N, term.evaluated_mask)
                case = (precision, kind, N, B, which, term.slab)
                for name, x, y in zip(NAMES, got, want):
                    assert same(x, y), (name, case)
                st = term.last_stats
                assert st["rays"] == B and st["samples"] == B * N and st["evaluated"] == int(ev.sum()) <= st["live"], case
                assert st["host_reads"] <= T.slab_count(N, term.slab) + 1 and st["network_launches"] <= st["slabs_run"], case
                assert term.transmittance.shape == (B, T.slab_count(N, term.slab)) and (term.transmittance[:, 0] == 1).all(), case
                assert st["terminated_rays"] == int((term.transmittance[:, -1] < term.eps).sum()), case
                dropped += st["live"] - st["evaluated"]
                if which is None:
                    assert st["live"] == B * N
                    with torch.no_grad():
                        explicit = render_nerf(rays, net, N, u=u, occupancy=grid(dev, "all"), terminate=term)
                    for name, x, y in zip(NAMES, got, explicit):
                        assert same(x, y), ("occupancy=None is the all-live grid", name, case)
    assert dropped > 0, "nothing was ever dropped"
    from nerf_simple_amd.utils.nets import packed_status
    if code != _lib.F32:
        assert packed_status(net.packed_weights(code), code) == 0


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_render_view_with_termination(dev, oracle, synthetic, precision):
    from nerf_simple_amd.utils.occupancy import EarlyTermination
    from nerf_simple_amd.utils.rendering import generate_rays, render_nerf, render_view
    net = make_net(dev, "structured", precision)
    pose = T.view(oracle, synthetic, 64, n_side=32)[0].numpy()
    cam = [32, 32, synthetic.focal_from_fov(32)]
    N = 64
    u_all = T.view(oracle, synthetic, N, n_side=32)[2]
    for which, eps in ((None, 0.1), ("ball-empty", 0.5), ("ball-live", 0.5)):
        occ = None if which is None else grid(dev, which)
        for ray0, n in ((0, 1024), (377, 250)):
            rays = generate_rays(pose, cam, dev, ray0, n)
            u = u_all[ray0:ray0 + n].contiguous().to(dev)
            with torch.no_grad():
                for kw in (dict(device_rng=True, seed=11), dict(u=u)):
                    t1, t2 = EarlyTermination(eps, 32), EarlyTermination(eps, 32)
                    px = render_view(net, pose, cam, N=N, ray0=ray0, n_rays=n, precision=precision, occupancy=occ, terminate=t1, **kw)
                    rgb, disp, _, acc, _ = render_nerf(rays, net, N, precision=precision, ray_id0=ray0, occupancy=occ, terminate=t2,
                                                       outputs=("rgb", "disp", "acc"), **kw)
                    assert t1.last_stats["evaluated"] == t2.last_stats["evaluated"] < t1.last_stats["live"], (which, ray0)
                    assert torch.equal(t1.evaluated_mask, t2.evaluated_mask)
                    assert same(px, torch.cat([rgb.clamp(0., 1.), disp[:, None]], 1)), (precision, which, ray0)


# ---- 3. no termination, no change -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_nothing_terminates_nothing_changes(dev, oracle, synthetic, precision):
    from nerf_simple_amd.utils.occupancy import EarlyTermination
    from nerf_simple_amd.utils.rendering import render_nerf
    net = make_net(dev, "default", precision)
    N = 128
    _, rays, u, _, _, _ = T.view(oracle, synthetic, N)
    rays, u = rays.to(dev), u.to(dev)
    for which in ("all", "ball-empty"):
        for S in T.SLABS:
            term, occ = EarlyTermination(1e-4, S), grid(dev, which)
            with torch.no_grad():
                got = render_nerf(rays, net, N, u=u, occupancy=occ, terminate=term)
                want = render_nerf(rays, net, N, u=u, occupancy=occ)
            for name, x, y in zip(NAMES, got, want):
                assert same(x, y), (name, which, S)
            st = term.last_stats
            assert st["evaluated"] == st["live"] == occ.last_stats["live"] and st["terminated_rays"] == 0
            # one read for the mark and one per slab; behind the ball the loop stops as soon as no live sample remains
            K = T.slab_count(N, S)
            assert st["host_reads"] == K + 1 if which == "all" else 2 <= st["host_reads"] <= K + 1, (which, S, st)


# ---- 4. it terminates, and stays inside its bound -----------------------------------------------------------------------------
@pytest.mark.parametrize("which,eps", [("all", 0.1), ("ball-empty", 0.5)])
@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_it_terminates_and_stays_inside_its_bound(dev, oracle, synthetic, precision, which, eps):
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils.occupancy import EarlyTermination
    from nerf_simple_amd.utils.rendering import render_nerf
    net = make_net(dev, "structured", precision)
    code = _lib.precision_code(precision)
    N, S = 128, 32
    _, rays, u, _, _, _ = T.view(oracle, synthetic, N)
    rays, u = rays.to(dev), u.to(dev)
    B = rays.shape[0]
    term, occ = EarlyTermination(eps, S), grid(dev, which)
    with torch.no_grad():
        got = render_nerf(rays, net, N, u=u, occupancy=occ, terminate=term)
        base = render_nerf(rays, net, N, u=u, occupancy=occ)
    st = term.last_stats
    share = st["terminated_rays"] / B
    print(f"{precision} {which} eps={eps}: terminated share {share:.4f}, evaluated {st['evaluated']} of {st['live']} live, "
          f"{st['slabs_run']} slabs, {st['network_launches']} launches, {st['host_reads']} host reads")
    assert 0.1 <= share <= 0.9
    assert st["evaluated"] < st["live"] == occ.last_stats["live"]
    _, full, ev = composed(dev, net, code, rays, u, tbins(N, dev), 0, 0, 0, N, term.evaluated_mask)
    assert st["evaluated"] == int(ev.sum())
    live0 = torch.from_numpy(unpack(occ.mark(rays, N, u=u).mask, N)).to(dev)
    assert not (ev & ~live0).any()
    dropped = live0 & ~ev
    c = full[..., :3].abs().amax(-1)
    cmax = torch.where(dropped, c, torch.zeros_like(c)).amax(1)
    slack = 4 * N * 2.0 ** -24
    d_rgb = (got[0] - base[0]).abs().amax(1)
    d_acc = (got[3] - base[3]).abs()
    print(f"  max |d rgb| / bound {float((d_rgb / (eps * cmax).clamp_min(1e-30))[cmax > 0].max()):.4f}, max |d acc| {float(d_acc.max()):.5f}")
    assert (d_rgb <= eps * cmax + slack * max(1.0, float(c.max()))).all()
    assert (d_acc <= eps + slack).all()
    assert float(d_acc.max()) > 0
    assert (got[2][~ev] == 0).all() and (got[4][~ev] == 0).all()
    untouched = ~dropped.any(1)
    for name, x, y in zip(NAMES, got, base):
        assert same(x[untouched], y[untouched]), ("a ray that drops nothing is bit for bit what it was", name)


# ---- 5. the range guard, the refusals, an all-dead grid ---------------------------------------------------------------------
def test_fp16_range_guard_through_the_terminated_path(dev, oracle, synthetic):
    from nerf_simple_amd.utils.occupancy import EarlyTermination
    from nerf_simple_amd.utils.rendering import render_nerf
    sd = {k: v.clone() for k, v in synthetic.synthetic_state_dict(0, "structured").items()}
    gain = 1e5                               # function-preserving rescaling: the first hidden activations leave fp16's range
    sd["layers_0.0.weight"] *= gain
    sd["layers_0.0.bias"] *= gain
    sd["layers_0.2.weight"] /= gain
    net = make_net(dev, "structured", sd=sd)
    assert net.precision == "fp16"
    N = 64
    _, rays, u, _, _, _ = T.view(oracle, synthetic, N)
    rays, u = rays.to(dev), u.to(dev)
    occ, term = grid(dev, "ball-empty"), EarlyTermination(0.5, 32)
    with torch.no_grad():
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            got = render_nerf(rays, net, N, u=u, occupancy=occ, terminate=term)
        hits = [w for w in rec if "fp16 MFMA operands left their range" in str(w.message)]
        assert len(hits) == 1, [str(w.message) for w in rec]
        first = dict(term.last_stats)
        # the figures are the repeat's own (bf16 operands): at most one launch per slab, at most K + 1 reads
        assert first["live"] > 0 and 0 < first["network_launches"] <= first["slabs_run"] and first["host_reads"] <= N // 32 + 1
        assert set(first) == {"rays", "samples", "live", "evaluated", "terminated_rays", "slabs_run", "network_launches", "host_reads"}
        mask = term.evaluated_mask.clone()
        bf = render_nerf(rays, net, N, u=u, precision="bf16", occupancy=occ, terminate=term)
    for name, x, y in zip(NAMES, got, bf):
        assert same(x, y), name
    assert torch.equal(mask, term.evaluated_mask) and first == term.last_stats
    assert torch.isfinite(got[0]).all() and (got[3] > 0).any()


def test_refusals_leave_the_generator_alone_and_an_all_dead_grid_launches_nothing(dev, oracle, synthetic):
    from nerf_simple_amd.utils.nets import Nerf
    from nerf_simple_amd.utils.occupancy import EarlyTermination
    from nerf_simple_amd.utils.rendering import render_nerf, render_view
    pose, rays = T.view(oracle, synthetic, 16)[:2]
    rays = rays[:16].contiguous().to(dev)
    net = make_net(dev, "structured", "bf16")
    other_size = Nerf(6, 4, 256).to(dev)              # (nn.Linear's initialisers draw from the CPU generator: build it first)
    term = EarlyTermination(0.01, 16)
    state = torch.get_rng_state()
    for occ in (None, grid(dev, "ball-empty")):
        with pytest.raises(RuntimeError, match="inference only.*torch.no_grad"):
            render_nerf(rays, net, 16, occupancy=occ, terminate=term)                    # a trainable net, grad enabled
        with pytest.raises(RuntimeError, match="inference only"):
            render_view(net, pose.numpy(), [8, 8, synthetic.focal_from_fov(8)], N=16, occupancy=occ, terminate=term)
        with torch.no_grad():
            with pytest.raises(RuntimeError, match="default Nerf"):
                render_nerf(rays, other_size, 16, occupancy=occ, terminate=term)

            class Foreign:
                def forward(self, q):
                    return torch.zeros(q.shape[0], 4, device=q.device)
            with pytest.raises(RuntimeError, match="foreign nets"):
                render_nerf(rays, Foreign(), 16, occupancy=occ, terminate=term)
            with pytest.raises(TypeError, match="EarlyTermination"):
                render_nerf(rays, net, 16, occupancy=occ, terminate=0.01)
            with pytest.raises(RuntimeError, match="768"):
                render_nerf(rays, net, 769, device_rng=True, occupancy=occ, terminate=term)
    assert torch.equal(torch.get_rng_state(), state), "a refused call must not consume the CPU generator"
    assert term.last_stats is None
    with torch.no_grad():
        got = render_nerf(rays, net, 16, device_rng=True, occupancy=grid(dev, "dead"), terminate=term)
    st = term.last_stats
    assert st["live"] == st["evaluated"] == st["network_launches"] == st["slabs_run"] == 0 and st["host_reads"] == 2
    assert st["terminated_rays"] == 0
    assert (got[0] == 0).all() and (got[3] == 0).all() and torch.isnan(got[1]).all() and (got[2] == 0).all()


def test_the_scan_over_several_blocks_of_rays(dev, oracle, synthetic):
    """5041 rays: three partitions of the offsets scan (2048 rays each), the last one short"""
    from nerf_simple_amd import _lib
    lib = _lib.lib()
    N, S, eps = 65, 32, 0.5
    _, rays, u, _, _, _ = T.view(oracle, synthetic, N, n_side=71)
    rays, u = rays.to(dev), u.to(dev)
    B = rays.shape[0]
    assert B == 5041
    occ = grid(dev, "ball-live")
    m = occ.mark(rays, N, u=u)
    head = (_lib.ptr(rays), _lib.ptr(u), _lib.ptr(tbins(N, dev)), 0, 0, 0)
    gen = torch.Generator().manual_seed(9)
    raw_live = torch.rand(m.live, 4, generator=gen)
    # sigma ~ N(-2, 2): on the CPU model (termination_model.terminate on these rays, 47 % of the samples live) 40 % of the rays
    # are terminated by the last check at eps = 0.5 (sigma ~ N(-3, 2): 5 %; N(-1, 2): 78 %)
    raw_live[:, 3] = torch.randn(m.live, generator=gen) * 2.0 - 2.0
    raw_live = raw_live.to(dev)
    raw0, trans, evaluated, live0, row0, intact, everything = drive(dev, lib, head, m, raw_live, eps, S, B, N)
    assert intact and 0 < evaluated.sum() < live0.sum()
    term = trans.cpu().numpy() < eps
    assert 0.1 < term[:, -1].mean() < 0.9
    again = drive(dev, lib, head, m, raw_live, eps, S, B, N)[-1]
    assert all(torch.equal(a, b) for a, b in zip(everything, again))


@pytest.mark.parametrize("S", T.SLABS)
def test_trans_is_the_masked_compositors_own_transmittance_bit_for_bit(dev, oracle, synthetic, S):
    """Pins the kernel's factor and scan to composite_ray's.  The compositor forms w = mul_rn(alpha, T): where alpha is exactly 1,
    w IS its transmittance.  So with nothing terminated, trans[:, k] must be, bit for bit, the w that
    nerf_amd_volume_render_masked gives sample k S when that one sample is made opaque (sigma = 1e6: alpha = 1 exactly at any
    delta here) and every earlier row is left as it is -- inside a 64-chunk and on chunk boundaries, where T is the carry."""
    from nerf_simple_amd import _lib
    lib = _lib.lib()
    occ = grid(dev, "all")
    eps = 1e-30
    for N in (65, 128, 192):
        _, rays_all, u_all, _, _, _ = T.view(oracle, synthetic, N)
        idx = subset(rays_all.shape[0], 37)
        rays, u = rays_all[idx].contiguous().to(dev), u_all[idx].contiguous().to(dev)
        B = rays.shape[0]
        m = occ.mark(rays, N, u=u)
        assert m.live == B * N
        head = (_lib.ptr(rays), _lib.ptr(u), _lib.ptr(tbins(N, dev)), 0, 0, 0)
        gen = torch.Generator().manual_seed(40 + N + S)
        raw_live = torch.rand(B * N, 4, generator=gen)
        raw_live[:, 3] = torch.randn(B * N, generator=gen)            # optical depth about 4 softplus(sigma) ~ 3: T stays far above eps
        raw_live = raw_live.to(dev)
        raw0, trans, evaluated, live0, row0, intact, _ = drive(dev, lib, head, m, raw_live, eps, S, B, N)
        assert intact and evaluated.all() and float(trans.min()) > 1e-6, "nothing may terminate here"
        for k in range(1, T.slab_count(N, S)):
            mod = raw_live.clone()
            mod.view(B, N, 4)[:, k * S, 3] = 1e6
            outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in ((B, 3), (B,), (B, N), (B,), (B, N))]
            _lib.check(lib.nerf_amd_volume_render_masked(_lib.ptr(mod), *head, _lib.ptr(m.mask), _lib.ptr(m.offsets),
                                                         *[_lib.ptr(o) for o in outs], B, N, _lib.stream_ptr(dev)), "masked")
            assert (outs[2][:, k * S] == 1).all(), (N, S, k)
            assert same(trans[:, k].contiguous(), outs[4][:, k * S].contiguous()), (N, S, k)
