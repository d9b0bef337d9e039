"""The masked hierarchical pair on the GPU (csrc/occupancy_graph.hip, csrc/occupancy_train.hip, training.train_step_hierarchical(occupancy=),
training.GraphedMaskedHierarchicalTrainStep, rendering.render_hierarchical[_view](occupancy=)).
Yardsticks: tests/occupancy_hierarchical_model.py on the occupancy / graphed models.

Kernel level: nerf_amd_volume_render_masked_mse_backward_pdf against the four existing entry points run under a host-built
mask_C / offsets_C (nerf_amd_volume_render_masked -> nerf_amd_mse_loss -> nerf_amd_volume_render_masked_backward ->
nerf_amd_sample_pdf): rgb, ts_out and d_raw bit for bit (every kernel of the chain runs
csrc/composite_backward_device.h), surplus rows exactly zero.  Device sampler against device sampler: no ray is excluded.  Step level: losses bit-equal
to the eager masked pair step, gradients within the dW products' run-to-run tolerance (1e-5 of the tensor's scale).  Trajectory: the criteria of
tests/test_gpu_training.py::test_graphed_train_step_matches_eager.  Inference: bit for bit against the dense pair (all-live
grid) and against the composition of the existing entry points (ball grid).

Every capacity is derived from a live count -- the CPU model's for the coarse pass, the eager reference step's for the fine
pass (its positions come out of the sampler) -- never typed in.
"""
import warnings

import numpy as np
import pytest
import torch

import occupancy_graphed_model as G
import occupancy_hierarchical_model as H
import occupancy_model as M
import occupancy_train_model as T

pytestmark = pytest.mark.gpu

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R129 = (129, 129, 129)
KERNEL_BS = (1, 37, 300)
# the sort's keys-per-lane buckets (E = 1, 2, 2, 1, 4, 4) and the compositor's 64-lane chunk seams; (64, 448) adds E = 8 at
# Nc + Nf = 512
KERNEL_SHAPES = ((3, 1), (64, 128), (66, 65), (67, 64), (130, 129), (256, 256), (64, 448))
POLICIES = ("empty", "live")
SENTINEL = 1234.5
NAMES = ("rgb", "disp", "alpha", "acc", "w")
_scene = {}


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


def make_net(dev, kind, precision="bf16", sd=None, seed=0):
    from nerf_simple_amd.utils import synthetic
    from nerf_simple_amd.utils.nets import Nerf
    net = Nerf(precision=precision).to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(seed, kind) if sd is None else sd)
    return net


def full_rays(oracle, synthetic):
    if "rays" not in _scene:
        pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, 30, 45))).float()
        _scene["rays"] = oracle.camera_rays(pose, [100, 100, synthetic.focal_from_fov(100)]).contiguous()
    return _scene["rays"]


def full_u(N, salt=0):
    if ("u", N, salt) not in _scene:
        _scene[("u", N, salt)] = torch.rand(10000, N, generator=torch.Generator().manual_seed(salt))
    return _scene[("u", N, salt)]


def subset(B):
    return np.array([5050]) if B == 1 else np.linspace(0, 9999, B).astype(np.int64)


def ball_grid(dev, outside):
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    key = ("grid", outside)
    if key not in _scene:
        _scene[key] = OccupancyGrid.from_mask(torch.from_numpy(M.ball_cells(R129, BOUNDS, 1.0)).to(dev), BOUNDS, outside=outside)
    return _scene[key]


def all_live_grid(dev):
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    if "all_live" not in _scene:
        _scene["all_live"] = OccupancyGrid.from_mask(torch.ones((16, 16, 16), dtype=torch.bool, device=dev), BOUNDS, outside="live")
    return _scene["all_live"]


def tbins(N, dev):
    from nerf_simple_amd.utils.rendering import _tbins
    return _tbins(2, 6, N, dev)


def query_points(rays, jit, tb, flags, seed, ray_id0, N):
    from nerf_simple_amd.utils.rendering import _query_points
    return _query_points(rays, jit, tb, flags, seed, ray_id0, N)


def model_live(rays, args, N, outside, cells=None):
    """the CPU model's verdict (T.live_of) on the sample positions the kernels form for these jitter arguments"""
    q, _ = query_points(rays, *args, N)
    cells = M.ball_cells(R129, BOUNDS, 1.0) if cells is None else cells
    R = tuple(c + 1 for c in cells.shape)
    return T.live_of(q.view(rays.shape[0], N, 6).cpu(), cells, R, BOUNDS, outside)


def to_dev_mask(kept, dev):
    """bool [B, N] -> (mask words int64 [B, W], offsets int64 [B + 1]) on the device"""
    words = torch.from_numpy(M.mask_words(kept).view(np.int64).copy()).to(dev)
    return words, torch.from_numpy(M.offsets(kept)).to(dev)


def jitter_args(mode, rays, u, N, dev):
    """(mark keywords, the reference kernels' coarse jitter arguments, the new kernel's, the sampler's (flags, seed, ray_id0))"""
    from nerf_simple_amd import _lib
    tb = tbins(N, dev)
    if mode == "u":
        return dict(u=u), (u, tb, 0, 0, 0), (u, tb, 0, 0, 0), (0, 0, 0)
    if mode == "ts":
        _, ts_in = query_points(rays, u, tb, 0, 0, 0, N)
        a = (ts_in, None, _lib.FLAG_TS_GIVEN, 0, 0)
        return dict(ts=ts_in), a, a, (0, 0, 0)
    # the new kernel takes the seed as a graph node does: 4 + an offset of 3 read from device memory
    off = torch.tensor([3], dtype=torch.int64, device=dev)
    return (dict(device_rng=True, seed=7, ray_id0=12345), (None, tb, _lib.FLAG_DEVICE_RNG, 7, 12345),
            (off, tb, _lib.FLAG_DEVICE_RNG | _lib.FLAG_SEED_IN_MEMORY, 4, 12345), (_lib.FLAG_DEVICE_RNG, 7, 12345))


def new_head(raw, rays, args, mask, offsets, gt, u_f, C, B, Nc, Nf, dev, pad=8):
    """-> (rgb [B, 3], the whole sentinel-prefilled d_raw buffer [C + pad, 4], the sentinel-prefilled flat ts_out buffer)"""
    from nerf_simple_amd import _lib
    jit, tb, flags, seed, rid = args
    rgb = torch.full((B, 3), SENTINEL, dtype=torch.float32, device=dev)
    buf = torch.full((C + pad, 4), SENTINEL, dtype=torch.float32, device=dev)
    ts_out = torch.full((B * (Nc + Nf) + pad,), SENTINEL, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().nerf_amd_volume_render_masked_mse_backward_pdf(
        _lib.ptr(raw), _lib.ptr(rays), _lib.ptr(jit), _lib.ptr(tb), flags, seed, rid, _lib.ptr(mask), _lib.ptr(offsets),
        _lib.ptr(gt), _lib.ptr(u_f), _lib.ptr(rgb), _lib.ptr(buf), _lib.ptr(ts_out), C, B, Nc, Nf, _lib.stream_ptr(dev)),
        "masked coarse head")
    return rgb, buf, ts_out


def reference_head(raw_kept, rays, args, mask_c, offsets_c, gt, u_f, sampler, B, Nc, Nf, dev):
    """the four existing entry points under mask_C / offsets_C: masked compositor (rgb, w) -> MSE gradient -> masked compositor
    backward -> sample_pdf on (ts_c, w)"""
    from nerf_simple_amd import _lib
    lib = _lib.lib()
    jit, tb, flags, seed, rid = args
    K = raw_kept.shape[0]
    st = _lib.stream_ptr(dev)
    rgb = torch.empty((B, 3), dtype=torch.float32, device=dev)
    disp, acc = torch.empty(B, device=dev), torch.empty(B, device=dev)
    w = torch.empty((B, Nc), dtype=torch.float32, device=dev)
    head = (_lib.ptr(raw_kept) if K else None, _lib.ptr(rays), _lib.ptr(jit), _lib.ptr(tb), flags, seed, rid, _lib.ptr(mask_c),
            _lib.ptr(offsets_c))
    _lib.check(lib.nerf_amd_volume_render_masked(*head, _lib.ptr(rgb), _lib.ptr(disp), None, _lib.ptr(acc), _lib.ptr(w), B, Nc, st),
               "masked compositor")
    loss, g = torch.empty((), device=dev), torch.empty((B, 3), device=dev)
    _lib.check(lib.nerf_amd_mse_loss(_lib.ptr(rgb), _lib.ptr(gt), _lib.ptr(loss), _lib.ptr(g), B * 3, st), "mse")
    d = torch.empty((K, 4), dtype=torch.float32, device=dev)
    _lib.check(lib.nerf_amd_volume_render_masked_backward(*head, _lib.ptr(g), None, None, None, None, _lib.ptr(d) if K else None,
                                                          B, Nc, st), "masked backward")
    ts_c = jit if flags & _lib.FLAG_TS_GIVEN else query_points(rays, jit, tb, flags, seed, rid, Nc)[1]
    sflags, sseed, srid = sampler
    ts_f = torch.empty((B, Nc + Nf), dtype=torch.float32, device=dev)
    _lib.check(lib.nerf_amd_sample_pdf(_lib.ptr(ts_c.contiguous()), _lib.ptr(w), None if sflags else _lib.ptr(u_f), sflags, sseed, srid,
                                       _lib.ptr(ts_f), B, Nc, Nf, st), "sample_pdf")
    return rgb, d, ts_f, w, ts_c


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["u", "ts", "device_rng"])
def test_masked_coarse_head_against_the_existing_entry_points(dev, oracle, synthetic, mode):
    rays_all = full_rays(oracle, synthetic).to(dev)
    gen = torch.Generator().manual_seed(17)
    overflowed, empty_rays = 0, 0
    for Nc, Nf in KERNEL_SHAPES:
        for B in KERNEL_BS:
            idx = torch.from_numpy(subset(B)).to(dev)
            rays = rays_all[idx].contiguous()
            u = full_u(Nc).to(dev)[idx].contiguous()
            u_f = full_u(Nf, salt=1).to(dev)[idx].contiguous()
            kw, ref_args, new_args, sampler = jitter_args(mode, rays, u, Nc, dev)
            gt = torch.rand(B, 3, generator=gen).to(dev)
            for outside in POLICIES:
                live = model_live(rays, ref_args, Nc, outside)
                total = int(live.sum())
                m = ball_grid(dev, outside).mark(rays, Nc, **kw)
                assert m.live == total, (mode, Nc, B, outside)
                raw_random = torch.randn(total, 4, generator=gen)
                raw_random[:, 3] *= 2.0
                # an opaque surface: every ray's weight sits on one sample (a peaked cdf for the sampler)
                raw_opaque = torch.rand(total, 4, generator=gen)
                raw_opaque[:, 3] = torch.where(torch.rand(total, generator=gen) < 0.3, 30.0, -30.0)
                caps = G.capacities(total, B, Nc)
                for kind, raw_live, cs in (("random", raw_random.to(dev), caps), ("opaque", raw_opaque.to(dev), caps[:1] + caps[4:5])):
                    for C in cs:
                        where = (mode, Nc, Nf, B, outside, kind, C, total)
                        kept = min(total, C)
                        kept_mask = G.mask_C(live, C)
                        mask_c, offsets_c = to_dev_mask(kept_mask, dev)
                        # raw[C, 4] with NaN in the surplus rows (never read)
                        raw = torch.full((C, 4), float("nan"), device=dev)
                        raw[:kept] = raw_live[:kept]
                        rgb_ref, d_ref, ts_ref, w_ref, ts_c = reference_head(raw_live[:kept].contiguous(), rays, ref_args, mask_c,
                                                                             offsets_c, gt, u_f, sampler, B, Nc, Nf, dev)
                        uf_new = None if sampler[0] else u_f
                        rgb, dbuf, tbuf = new_head(raw, rays, new_args, m.mask, m.offsets, gt, uf_new, C, B, Nc, Nf, dev)
                        rgb2, dbuf2, tbuf2 = new_head(raw, rays, new_args, m.mask, m.offsets, gt, uf_new, C, B, Nc, Nf, dev)
                        assert same(rgb, rgb2) and same(dbuf, dbuf2) and same(tbuf, tbuf2), where      # two runs, the same bytes
                        assert same(rgb, rgb_ref), where                                  # rgb bit for bit
                        ts_out = tbuf[:B * (Nc + Nf)].view(B, Nc + Nf)
                        assert same(ts_out, ts_ref), where                                # ts_out bit for bit
                        assert (tbuf[B * (Nc + Nf):] == SENTINEL).all(), where            # nothing beyond ts_out
                        assert (dbuf[kept:C] == 0).all() and (dbuf[C:] == SENTINEL).all(), where
                        got = dbuf[:kept]
                        assert torch.isfinite(d_ref).all() and torch.isfinite(got).all() and torch.isfinite(ts_out).all(), where
                        assert same(got, d_ref), where                                    # d_raw bit for bit
                        no_kept = torch.from_numpy(kept_mask.sum(1) == 0).to(dev)
                        assert (rgb[no_kept] == 0).all(), where                           # a ray with nothing kept
                        if bool(no_kept.any()):
                            # ... gets the sampler's uniform rows: what sample_pdf makes of zero weights
                            zero = reference_sampler(ts_c, torch.zeros_like(w_ref), u_f, sampler, B, Nc, Nf, dev)
                            assert same(ts_out[no_kept], zero[no_kept]), where
                            empty_rays += int(no_kept.sum())
                        assert (w_ref[torch.from_numpy(~kept_mask).to(dev)] == 0).all(), where
                        overflowed += int(total > C)
    assert empty_rays > 0 and overflowed > 0


def reference_sampler(ts_c, w, u_f, sampler, B, Nc, Nf, dev):
    from nerf_simple_amd import _lib
    sflags, sseed, srid = sampler
    out = torch.empty((B, Nc + Nf), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().nerf_amd_sample_pdf(_lib.ptr(ts_c.contiguous()), _lib.ptr(w), None if sflags else _lib.ptr(u_f), sflags, sseed,
                                              srid, _lib.ptr(out), B, Nc, Nf, _lib.stream_ptr(dev)), "sample_pdf")
    return out


# ---- 2. the step -----------------------------------------------------------------------------------------------------------
def make_pair(dev, kind, fine_seed=1):
    return make_net(dev, kind), make_net(dev, kind, seed=fine_seed)


def graphed_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf, cap, fine_seed=1, **kw):
    """one graphed masked pair step with lr = 0 -> (losses [2], (coarse gradients, fine gradients), the stepper)"""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedMaskedHierarchicalTrainStep
    net_c, net_f = make_pair(dev, kind, fine_seed)
    opt = FusedAdam([net_c, net_f], lr=0.0)
    stepper = GraphedMaskedHierarchicalTrainStep(net_c, net_f, opt, rays.shape[0], Nc, Nf, occ, cap, **kw)
    total = stepper.step(rays.to(dev), gt.to(dev), u_c=None if u_c is None else u_c.to(dev), u_f=None if u_f is None else u_f.to(dev))
    losses = stepper.losses.clone()
    assert same(total.clone(), losses[0] + losses[1])
    grads = tuple({k: p.grad.clone() for k, p in n.named_parameters()} for n in (net_c, net_f))
    return losses, grads, stepper


def eager_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf, C_c=None, C_f=None, fine_seed=1, **kw):
    """the eager masked pair step with lr = 0 -> (losses [2], (coarse gradients, fine gradients), info); with a capacity the
    existing autograd functions composed under mask_C.  info: live_c / live_f (bool [B, N] on the host) and ts_f."""
    from nerf_simple_amd import training
    from nerf_simple_amd.utils.rendering import sample_pdf
    net_c, net_f = make_pair(dev, kind, fine_seed)
    rays, gt, u_c, u_f = rays.to(dev), gt.to(dev), u_c.to(dev), u_f.to(dev)
    B = rays.shape[0]
    if C_c is None and C_f is None:
        opt = torch.optim.SGD(list(net_c.parameters()) + list(net_f.parameters()), lr=0.0)
        out = training.train_step_hierarchical(net_c, net_f, opt, rays, gt, Nc, Nf, u_c=u_c, u_f=u_f, occupancy=occ, **kw)
        losses, ts_f = torch.stack(out.losses), out.ts_f
        assert same(out, losses[0] + losses[1])
        info = dict(stats=occ.last_stats)
    else:
        info, losses, ts = {}, [], None
        for net, N, C in ((net_c, Nc, C_c), (net_f, Nc + Nf, C_f)):
            jit = dict(u=u_c) if ts is None else dict(ts=ts)
            m = occ.mark(rays, N, points=True, **jit)
            live = M_unpack(m.mask, N)
            kept_mask = live if C is None else G.mask_C(live, C)
            K = int(kept_mask.sum())
            mask_c, offsets_c = to_dev_mask(kept_mask, dev)
            params = [p for _, p in net.named_parameters()]
            raw, _ = training._FusedDense.apply(net, None, None, None, 0, 0, 0, 1, m.points[:K].contiguous(), *params)
            head = (rays, u_c, tbins(N, dev), 0, 0, 0, mask_c, offsets_c) if ts is None else \
                (rays, ts, None, 1, 0, 0, mask_c, offsets_c)
            outs = training._MaskedVolumeRender.apply(raw.reshape(-1, 4), head, B, N)
            loss = training.mse_loss(outs[0], gt)
            loss.backward()
            losses.append(loss.detach())
            if ts is None:
                ts_c = query_points(rays, u_c, tbins(N, dev), 0, 0, 0, N)[1]
                ts = sample_pdf(ts_c, outs[4].detach(), Nf, u=u_f)
        losses, ts_f = torch.stack(losses), ts
    info["ts_f"] = ts_f
    info["live_c"] = model_live(rays, (u_c, tbins(Nc, dev), 0, 0, 0), Nc, occ.outside, cells=info_cells(occ))
    info["live_f"] = model_live(rays, (ts_f, None, 1, 0, 0), Nc + Nf, occ.outside, cells=info_cells(occ))
    grads = tuple({k: p.grad for k, p in n.named_parameters()} for n in (net_c, net_f))
    return losses, grads, info


def info_cells(occ):
    return occ.cells().cpu().numpy()


def M_unpack(mask, N):
    """mask words int64 [B, W] on the device -> bool [B, N] on the host"""
    w = mask.cpu().numpy().view(np.uint64)
    i = np.arange(N)
    return ((w[:, i >> 6] >> (i & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def compare_gradients(got, want, where):
    # the run-to-run tolerance tests/test_gpu_training.py::test_ragged_training_ignores_garbage_beyond_P grants the dW products
    for g_, w_ in zip(got, want):
        for k, g in w_.items():
            scale = float(g.abs().max())
            assert float((g_[k] - g).abs().max()) <= 1e-5 * scale, (where, k, scale)


STEP_CASES = [(576, 64, 128, "empty"), (576, 66, 65, "live"), (37, 64, 128, "live"), (37, 66, 65, "empty")]


def up256(n, total):
    return min(-(-(n + 1) // 256) * 256, total)


@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("case", STEP_CASES)
def test_graphed_pair_step_is_the_eager_masked_pair_step(dev, oracle, synthetic, case, kind):
    B, Nc, Nf, outside = case
    rays, gt, u_c, u_f = H.pair_inputs(oracle, synthetic, B, Nc, Nf)
    occ = ball_grid(dev, outside)
    want_losses, want, info = eager_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf)
    live_c, live_f = info["live_c"], info["live_f"]
    M.require_informative(live_c, Nc, outside)
    Pc, Pf = int(live_c.sum()), int(live_f.sum())
    st = info["stats"]
    assert st["coarse"]["live"] == Pc and st["fine"]["live"] == Pf and st["live"] == Pc + Pf and st["rays"] == B
    assert st["samples"] == B * (Nc + Nc + Nf) and st["network_launches"] == 2
    print(f"{case} {kind}: live fraction coarse {Pc / (B * Nc):.3f}, fine {Pf / (B * (Nc + Nf)):.3f}")
    for cap in ((Pc, Pf), (up256(Pc, B * Nc), up256(Pf, B * (Nc + Nf)))):      # exactly the eager counts, and with surplus rows
        losses, grads, stepper = graphed_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf, cap)
        assert stepper.counts() == {"step": 1,
                                    "coarse": {"samples": B * Nc, "live": Pc, "kept": Pc, "capacity": cap[0]},
                                    "fine": {"samples": B * (Nc + Nf), "live": Pf, "kept": Pf, "capacity": cap[1]}}
        assert same(losses, want_losses), (case, kind, cap, losses.tolist(), want_losses.tolist())
        assert same(stepper.ts_f, info["ts_f"]), (case, kind, cap)
        if cap == (Pc, Pf):
            compare_gradients(grads, want, (case, kind, cap))
            exact = grads
        else:
            # the surplus rows add exact zeros to every product: the gradients are those of the exact capacities, to the
            # run-to-run tolerance tests/test_gpu_training.py::test_ragged_training_ignores_garbage_beyond_P grants the dW products
            for g_, w_ in zip(grads, exact):
                for k, g in w_.items():
                    assert float((g_[k] - g).abs().max()) <= 1e-5 * float(g.abs().max()), (case, kind, cap, k)


@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("case", [(576, 64, 128, "empty"), (37, 66, 65, "empty")])
def test_short_coarse_capacity_is_the_eager_composition_under_mask_C(dev, oracle, synthetic, case, kind):
    B, Nc, Nf, outside = case
    rays, gt, u_c, u_f = H.pair_inputs(oracle, synthetic, B, Nc, Nf)
    occ = ball_grid(dev, outside)
    live_c = model_live(rays.to(dev), (u_c.to(dev), tbins(Nc, dev), 0, 0, 0), Nc, outside)
    Pc = int(live_c.sum())
    C_c = -(-Pc // 2)
    assert C_c not in set(M.offsets(live_c).tolist())                                  # the capacity cuts inside a ray
    want_losses, want, info = eager_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf, C_c=C_c)
    full_losses, _, full = eager_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf)
    Pf = int(info["live_f"].sum())
    losses, grads, stepper = graphed_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf, (C_c, 1.0))
    now = stepper.counts()
    assert now["coarse"] == {"samples": B * Nc, "live": Pc, "kept": C_c, "capacity": C_c}
    assert now["fine"] == {"samples": B * (Nc + Nf), "live": Pf, "kept": Pf, "capacity": B * (Nc + Nf)}
    assert same(losses, want_losses), (case, kind, losses.tolist(), want_losses.tolist())
    assert same(stepper.ts_f, info["ts_f"]) and not same(stepper.ts_f, full["ts_f"])   # the sampler saw the stricter mask
    assert not same(losses[0], full_losses[0])                                          # the dropped tail did matter
    compare_gradients(grads, want, (case, kind, C_c))
    # a short FINE capacity likewise
    C_f = -(-int(full["live_f"].sum()) // 2)
    want_losses, want, info = eager_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf, C_f=C_f)
    losses, grads, stepper = graphed_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf, (1.0, C_f))
    assert stepper.counts()["fine"]["kept"] == C_f and stepper.counts()["coarse"]["kept"] == Pc
    assert same(losses, want_losses) and same(losses[0], full_losses[0]) and not same(losses[1], full_losses[1])


@pytest.mark.parametrize("kind", ["default", "structured"])
def test_coarse_gradients_are_the_single_masked_steps_whatever_the_fine_net(dev, oracle, synthetic, kind):
    """gradients stop at w: the coarse network's gradients (and loss) are train_step(net_c, ..., occupancy=occ)'s"""
    from nerf_simple_amd.training import train_step
    B, Nc, Nf, outside = 576, 64, 128, "empty"
    rays, gt, u_c, u_f = H.pair_inputs(oracle, synthetic, B, Nc, Nf)
    occ = ball_grid(dev, outside)
    net = make_net(dev, kind)
    loss = train_step(net, torch.optim.SGD(net.parameters(), lr=0.0), rays.to(dev), gt.to(dev), Nc, u=u_c.to(dev), occupancy=occ)
    single = {k: p.grad for k, p in net.named_parameters()}
    seen = []
    for fine_seed in (1, 2):
        losses, (g_c, g_f), _ = eager_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf, fine_seed=fine_seed)
        assert same(losses[0], loss)
        for k, g in single.items():
            assert float((g_c[k] - g).abs().max()) <= 1e-5 * float(g.abs().max()), (kind, fine_seed, k)
        seen.append(losses[1].clone())
        glosses, (gg_c, _), _ = graphed_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf, (1.0, 1.0), fine_seed=fine_seed)
        assert same(glosses, losses)
        for k, g in single.items():
            assert float((gg_c[k] - g).abs().max()) <= 1e-5 * float(g.abs().max()), (kind, fine_seed, k)
    assert not same(seen[0], seen[1])                                                   # the fine nets did differ


@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("shape", [(576, 64, 128), (37, 66, 65)])
def test_all_live_grid_is_the_dense_points_mode_pair_step(dev, oracle, synthetic, shape, kind):
    from nerf_simple_amd.training import mse_loss, nerf_forward_autograd, volume_render_autograd
    from nerf_simple_amd.utils.rendering import sample_pdf
    B, Nc, Nf = shape
    rays, gt, u_c, u_f = H.pair_inputs(oracle, synthetic, B, Nc, Nf)
    occ = all_live_grid(dev)
    losses, _, info = eager_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf)
    assert info["stats"]["coarse"]["live"] == B * Nc and info["stats"]["fine"]["live"] == B * (Nc + Nf)
    # the dense pair step with both forwards in points mode, on the same jitter
    net_c, net_f = make_pair(dev, kind)
    r = rays.to(dev)
    q, ts_c = query_points(r, u_c.to(dev), tbins(Nc, dev), 0, 0, 0, Nc)
    dirs = q.view(B, Nc, 6)[:, 0, 3:6].contiguous()
    coarse = volume_render_autograd(nerf_forward_autograd(net_c, q, "bf16").reshape(B, Nc, 4), ts_c, dirs)
    ts_f = sample_pdf(ts_c, coarse[4].detach(), Nf, u=u_f.to(dev))
    q_f, _ = query_points(r, ts_f, None, 1, 0, 0, Nc + Nf)
    fine = volume_render_autograd(nerf_forward_autograd(net_f, q_f, "bf16").reshape(B, Nc + Nf, 4), ts_f, dirs)
    want = torch.stack([mse_loss(coarse[0], gt.to(dev)).detach(), mse_loss(fine[0], gt.to(dev)).detach()])
    assert same(info["ts_f"], ts_f)
    assert same(losses, want), (losses.tolist(), want.tolist())
    # ... and the graphed step at full capacity gives the same
    glosses, _, _ = graphed_step(dev, kind, occ, rays, gt, u_c, u_f, Nc, Nf, (1.0, 1.0))
    assert same(glosses, want)


def test_all_dead_batch(dev, oracle, synthetic):
    B, Nc, Nf = 576, 64, 128
    rays, gt, u_c, u_f = H.pair_inputs(oracle, synthetic, B, Nc, Nf)
    away = torch.cat([rays[:, :3], -rays[:, 3:]], 1).contiguous()       # the camera looks away from the grid
    assert not model_live(away.to(dev), (u_c.to(dev), tbins(Nc, dev), 0, 0, 0), Nc, "empty").any()
    occ = ball_grid(dev, "empty")
    want = float((gt.double() ** 2).mean())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        losses, grads, stepper = graphed_step(dev, "default", occ, away, gt, u_c, u_f, Nc, Nf, (0.25, 0.25))
        assert stepper.capacity == (B * Nc // 4, B * (Nc + Nf) // 4)
        now = stepper.counts()
        assert (now["coarse"]["live"], now["coarse"]["kept"], now["fine"]["live"], now["fine"]["kept"]) == (0, 0, 0, 0)
        elosses, egrads, info = eager_step(dev, "default", occ, away, gt, u_c, u_f, Nc, Nf)
    assert info["stats"]["network_launches"] == 0 and same(losses, elosses)
    total = float(losses[0] + losses[1])
    assert abs(total - 2 * want) <= 1e-6 * 2 * want, (total, 2 * want)      # loss = 2 mean(gt^2): fp32 sums of 3 B squares
    # every ray had nothing kept: the fine positions are the sampler's uniform rows
    ts_c = query_points(away.to(dev), u_c.to(dev), tbins(Nc, dev), 0, 0, 0, Nc)[1]
    uniform = reference_sampler(ts_c, torch.zeros_like(ts_c), u_f.to(dev), (0, 0, 0), B, Nc, Nf, dev)
    assert same(stepper.ts_f, uniform) and same(info["ts_f"], uniform)
    for gs in grads + egrads:
        for k, g in gs.items():
            assert (g == 0).all(), k


# ---- 3. trajectories ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_rng", [False, True])
def test_graphed_masked_pair_trajectory_matches_eager(dev, oracle, synthetic, device_rng):
    """6 decayed FusedAdam steps, graphed against eager masked pair, under the criteria of
    tests/test_gpu_training.py::test_graphed_train_step_matches_eager; the six replays run with no host sync between them.
    The capacities come from the eager run's own counts, rounded up to 256: the coarse count depends on the jitter alone; the
    fine count follows the weights, which the two runs share only to the trajectory tolerance, hence 5 % of headroom."""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedMaskedHierarchicalTrainStep, lr_decay_factor, train_step_hierarchical
    B, Nc, Nf, seed = 576, 64, 128, 40
    rays, gt, _, _ = H.pair_inputs(oracle, synthetic, B, Nc, Nf)
    rays, gt = rays.to(dev), gt.to(dev)
    occ = ball_grid(dev, "empty")
    decay = lr_decay_factor(5e-4, 4e-4, 10)
    ucs = [torch.rand(B, Nc, generator=torch.Generator().manual_seed(100 + i)).to(dev) for i in range(6)]
    ufs = [torch.rand(B, Nf, generator=torch.Generator().manual_seed(200 + i)).to(dev) for i in range(6)]
    runs, counts, cap = [], [], None
    for graphed in (False, True):
        net_c, net_f = make_pair(dev, "default")
        opt = FusedAdam([net_c, net_f], lr=5e-4)
        if graphed:
            stepper = GraphedMaskedHierarchicalTrainStep(net_c, net_f, opt, B, Nc, Nf, occ, cap, device_rng=device_rng, seed=seed,
                                                         check_every=2)
            torch.cuda.synchronize()
            with warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)                   # an overflow report would raise
                held = [stepper.step(rays, gt, u_c=None if device_rng else ucs[i], u_f=None if device_rng else ufs[i],
                                     decay=decay).clone() for i in range(6)]
            losses = [float(x) for x in held]
            assert opt.step_count == 6 and stepper.overflow_steps == 0
            now = stepper.counts()
            assert now["coarse"]["live"] == counts[-1][0]                        # the coarse count depends on the jitter only
            assert abs(now["fine"]["live"] - counts[-1][1]) <= 0.05 * counts[-1][1]
            assert stepper.last_stats["coarse"]["live"] == counts[stepper.last_stats["step"] - 1][0]
        else:
            kw = [dict(device_rng=True, seed=seed + k) for k in range(1, 7)] if device_rng else \
                [dict(u_c=a, u_f=b) for a, b in zip(ucs, ufs)]
            losses = []
            for i in range(6):
                losses.append(float(train_step_hierarchical(net_c, net_f, opt, rays, gt, Nc, Nf, decay=decay, occupancy=occ, **kw[i])))
                counts.append((occ.last_stats["coarse"]["live"], occ.last_stats["fine"]["live"]))
            cap = (up256(max(c for c, _ in counts), B * Nc), up256(int(1.05 * max(f for _, f in counts)), B * (Nc + Nf)))
        assert abs(opt.param_groups[0]["lr"] - 5e-4 * decay ** 6) < 1e-12
        with torch.no_grad():
            probe = torch.cat([n(rays[:8].new_zeros(8, 6) + 0.1).cpu() for n in (net_c, net_f)])
        runs.append((losses, torch.cat([p.detach().reshape(-1) for n in (net_c, net_f) for p in n.parameters()]).cpu(), probe))
    (la, pa, qa), (lb, pb, qb) = runs
    print(f"pair trajectory device_rng={device_rng}: eager {la} graphed {lb}; capacities {cap} for live counts {counts}")
    assert la[-1] < la[0] and lb[-1] < lb[0]
    np.testing.assert_allclose(la, lb, rtol=2e-3)
    d = (pa - pb).abs()
    assert float(d.max()) <= 6 * 5e-4 and float(d.mean()) <= 1e-5 and float((d > 1e-5).float().mean()) <= 0.06
    assert float((qa - qb).abs().max()) <= 2e-2 * max(1.0, float(qa.abs().max()))


def test_graphed_masked_pair_step_selects_its_own_rays(dev, oracle, synthetic):
    """rays_from with device_rng=True: the next batch is selected on graph A's side branch.  Every replay trains on the
    oracle's batch for (seed, step) and, with lr = 0, gives the losses of the same stepper fed by hand and of the eager
    masked pair step on that batch, bit for bit."""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedMaskedHierarchicalTrainStep, train_step_hierarchical
    from nerf_simple_amd.utils.dataload import RayGenerator
    rays_tab = full_rays(oracle, synthetic)
    gt_tab = torch.rand(rays_tab.shape[0], 3, generator=torch.Generator().manual_seed(21))
    n, B, Nc, Nf, seed = rays_tab.shape[0], 576, 64, 128, 11
    rg = RayGenerator.from_tables(rays_tab, gt_tab, device=dev)
    occ = ball_grid(dev, "empty")
    cap = (0.5, 0.5)
    pairs = [make_pair(dev, "structured") for _ in range(3)]
    auto = GraphedMaskedHierarchicalTrainStep(*pairs[0], FusedAdam(list(pairs[0]), lr=0.0), B, Nc, Nf, occ, cap, device_rng=True,
                                              seed=seed, rays_from=rg)
    hand = GraphedMaskedHierarchicalTrainStep(*pairs[1], FusedAdam(list(pairs[1]), lr=0.0), B, Nc, Nf, occ, cap, device_rng=True,
                                              seed=seed)
    eager_opt = torch.optim.SGD([p for m in pairs[2] for p in m.parameters()], lr=0.0)
    for step in (1, 2, 3):
        auto.step()
        la = auto.losses.clone()
        want = torch.from_numpy(oracle.select_ids_counter(n, B, seed, step))
        assert torch.equal(auto.ray_ids.cpu(), want), step
        rays, gt = rays_tab[want].to(dev), gt_tab[want].to(dev)
        hand.step(rays, gt)
        lb = hand.losses.clone()
        out = train_step_hierarchical(*pairs[2], eager_opt, rays, gt, Nc, Nf, device_rng=True, seed=seed + step, occupancy=occ)
        le = torch.stack(out.losses)
        st = occ.last_stats
        now = auto.counts()
        assert st["coarse"]["live"] <= auto.capacity[0] and st["fine"]["live"] <= auto.capacity[1]
        assert (now["coarse"]["live"], now["fine"]["live"]) == (st["coarse"]["live"], st["fine"]["live"]), step
        assert same(la, lb) and same(la, le), (step, la.tolist(), lb.tolist(), le.tolist())
    with pytest.raises(RuntimeError):
        auto.step(rays_tab[:B].to(dev), gt_tab[:B].to(dev))


# ---- 4. the grid and the reports ---------------------------------------------------------------------------------------
def test_grid_update_between_replays_and_replaced_words(dev, oracle, synthetic):
    from nerf_simple_amd.utils import mesh
    from nerf_simple_amd.utils.occupancy import TrainingOccupancyGrid
    B, Nc, Nf, R = 576, 64, 128, (33, 33, 33)
    rays, gt, u_c, u_f = H.pair_inputs(oracle, synthetic, B, Nc, Nf)
    occ = TrainingOccupancyGrid(R, BOUNDS, outside="empty", device=dev)
    losses, _, stepper = graphed_step(dev, "structured", occ, rays, gt, u_c, u_f, Nc, Nf, (1.0, 1.0))
    first = stepper.counts()
    before = model_live(rays.to(dev), (u_c.to(dev), tbins(Nc, dev), 0, 0, 0), Nc, "empty", cells=np.ones((32, 32, 32), bool))
    assert first["coarse"]["live"] == int(before.sum()) == first["coarse"]["kept"]
    # the grid follows the FINE network; update() writes the bits in place: the next replay sees them
    sigma = mesh.density_grid(stepper.net_f, R, BOUNDS).cpu().numpy()
    level = float(np.percentile(sigma, 90))
    words_ptr = occ.words.data_ptr()
    occ.update(stepper.net_f, level, decay=0.5, dilate=1)
    assert occ.words.data_ptr() == words_ptr
    cells = T.cells_from_state(occ.state.cpu().numpy(), level, 1)
    assert np.array_equal(cells, occ.cells().cpu().numpy())
    stepper.step(rays.to(dev), gt.to(dev), u_c=u_c.to(dev), u_f=u_f.to(dev))
    losses2 = stepper.losses.clone()
    want, _, info = eager_step(dev, "structured", occ, rays, gt, u_c, u_f, Nc, Nf)      # lr = 0: the same weights
    Pc, Pf = int(info["live_c"].sum()), int(info["live_f"].sum())
    print(f"grid update: coarse live {first['coarse']['live']} -> {Pc}, fine live {first['fine']['live']} -> {Pf}")
    assert 0.02 < Pc / (B * Nc) < 0.6
    now = stepper.counts()
    assert now["step"] == 2 and (now["coarse"]["live"], now["coarse"]["kept"], now["fine"]["live"], now["fine"]["kept"]) == (Pc, Pc, Pf, Pf)
    assert Pc != first["coarse"]["live"] and Pf != first["fine"]["live"]                # all four counts changed
    assert same(losses2, want), (losses2.tolist(), want.tolist())
    assert not same(losses2[0], losses[0]) and not same(losses2[1], losses[1])
    # a replaced words tensor is refused: its address is baked into the graph
    occ.words = occ.words.clone()
    with pytest.raises(RuntimeError, match="words"):
        stepper.step(rays.to(dev), gt.to(dev), u_c=u_c.to(dev), u_f=u_f.to(dev))
    assert stepper.opt.step_count == 2


@pytest.mark.parametrize("short", ["coarse", "fine"])
def test_overflow_is_reported_with_the_pass(dev, oracle, synthetic, short):
    B, Nc, Nf = 576, 64, 128
    rays, gt, u_c, u_f = H.pair_inputs(oracle, synthetic, B, Nc, Nf)
    occ = ball_grid(dev, "empty")
    _, _, info = eager_step(dev, "default", occ, rays, gt, u_c, u_f, Nc, Nf)
    Pc, Pf = int(info["live_c"].sum()), int(info["live_f"].sum())
    total, C = (Pc, -(-Pc // 2)) if short == "coarse" else (Pf, -(-Pf // 2))
    cap = (C, 1.0) if short == "coarse" else (1.0, C)
    r, g, a, b = rays.to(dev), gt.to(dev), u_c.to(dev), u_f.to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        _, _, stepper = graphed_step(dev, "default", occ, rays, gt, u_c, u_f, Nc, Nf, cap, check_every=1)
    assert stepper.last_stats is None and stepper.overflow_steps == 0          # nothing polled yet
    torch.cuda.synchronize()
    with pytest.warns(RuntimeWarning, match=rf"step 1: the {short} pass had {total} live samples for a capacity of {C} points") as rec:
        stepper.step(r, g, u_c=a, u_f=b)
    other = "fine" if short == "coarse" else "coarse"
    assert not any(f"the {other} pass" in str(w.message) for w in rec)
    assert stepper.overflow_steps == 1 and stepper.last_stats["step"] == 1
    assert stepper.last_stats[short] == {"samples": B * (Nc if short == "coarse" else Nc + Nf), "live": total, "kept": C, "capacity": C}
    assert stepper.last_stats[other]["live"] == stepper.last_stats[other]["kept"]
    with pytest.warns(RuntimeWarning, match="step 2"):
        now = stepper.counts()                                                 # delivers the pending report, then reads
    assert now["step"] == 2 and now[short]["kept"] == C and now[short]["live"] == total
    assert stepper.overflow_steps == 2 and stepper.last_stats["step"] == 2


def test_refusals_leave_the_generator_untouched(dev, oracle, synthetic):
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedMaskedHierarchicalTrainStep as Step, train_step_hierarchical
    from nerf_simple_amd.utils.nets import Nerf
    from nerf_simple_amd.utils.rendering import render_hierarchical, render_hierarchical_view
    B, Nc, Nf = 37, 66, 65
    occ = ball_grid(dev, "live")
    net_c, net_f = make_pair(dev, "default")
    opt = FusedAdam([net_c, net_f], lr=5e-4)

    class Foreign:
        precision = "bf16"

        def forward(self, q):
            return torch.zeros(q.shape[0], 4, device=q.device)

    # every input is built BEFORE the generator is read: nn.Linear's initialisation draws from it
    fp32_c, fp32_f = make_net(dev, "default", "fp32"), make_net(dev, "default", "fp32", seed=1)
    small = Nerf(6, 4, 128, precision="bf16").to(dev)
    other = FusedAdam([make_net(dev, "default"), make_net(dev, "default")], lr=5e-4)
    single = FusedAdam(make_net(dev, "default"), lr=5e-4)
    rays, gt, u_c, u_f = (t.to(dev) for t in H.pair_inputs(oracle, synthetic, B, Nc, Nf))
    grad_rays = rays.clone().requires_grad_(True)
    sgd = torch.optim.SGD(list(net_c.parameters()) + list(net_f.parameters()), lr=0.0)
    pose = oracle.spherical_to_pose(4, 30, 45)
    cam = [6, 6, synthetic.focal_from_fov(6)]
    half = (0.5, 0.5)
    cases = [
        ("storage='e4m3'", ValueError, lambda: Step(net_c, net_f, opt, B, Nc, Nf, occ, half, storage="e4m3")),
        ("buckets=2", ValueError, lambda: Step(net_c, net_f, opt, B, Nc, Nf, occ, half, buckets=2)),
        ("Nc + Nf > 512", ValueError, lambda: Step(net_c, net_f, opt, B, 256, 257, occ, half)),
        ("Nc < 3", ValueError, lambda: Step(net_c, net_f, opt, B, 2, 8, occ, half)),
        ("fp32 modules", RuntimeError, lambda: Step(fp32_c, fp32_f, None, B, Nc, Nf, occ, half)),
        ("another network size", RuntimeError, lambda: Step(net_c, small, None, B, Nc, Nf, occ, half)),
        ("a foreign net", RuntimeError, lambda: Step(Foreign(), net_f, None, B, Nc, Nf, occ, half)),
        ("not a grid", TypeError, lambda: Step(net_c, net_f, opt, B, Nc, Nf, object(), half)),
        ("another pair's optimizer", RuntimeError, lambda: Step(net_c, net_f, other, B, Nc, Nf, occ, half)),
        ("a single module's optimizer", RuntimeError, lambda: Step(net_c, net_f, single, B, Nc, Nf, occ, half)),
        ("no capacity", TypeError, lambda: Step(net_c, net_f, opt, B, Nc, Nf, occ)),
        ("one capacity", TypeError, lambda: Step(net_c, net_f, opt, B, Nc, Nf, occ, 0.5)),
        ("coarse capacity 0", ValueError, lambda: Step(net_c, net_f, opt, B, Nc, Nf, occ, (0, 0.5))),
        ("fine capacity beyond B (Nc + Nf)", ValueError, lambda: Step(net_c, net_f, opt, B, Nc, Nf, occ, (0.5, B * (Nc + Nf) + 1))),
        ("a fraction beyond 1", ValueError, lambda: Step(net_c, net_f, opt, B, Nc, Nf, occ, (1.5, 0.5))),
        ("a capacity that is no number", TypeError, lambda: Step(net_c, net_f, opt, B, Nc, Nf, occ, ("half", 0.5))),
        ("eager: rays that require grad", RuntimeError, lambda: train_step_hierarchical(net_c, net_f, sgd, grad_rays, gt, Nc, Nf, occupancy=occ)),
        ("eager: fp32 modules", RuntimeError, lambda: train_step_hierarchical(
            fp32_c, fp32_f, torch.optim.SGD(list(fp32_c.parameters()) + list(fp32_f.parameters()), lr=0.0), rays, gt, Nc, Nf, occupancy=occ)),
        ("eager: precision='fp32'", RuntimeError, lambda: train_step_hierarchical(net_c, net_f, sgd, rays, gt, Nc, Nf, precision="fp32",
                                                                              occupancy=occ)),
        ("eager: not a grid", TypeError, lambda: train_step_hierarchical(net_c, net_f, sgd, rays, gt, Nc, Nf, occupancy="grid")),
        ("eager: Nc + Nf > 512", ValueError, lambda: train_step_hierarchical(net_c, net_f, sgd, rays, gt, 256, 257, occupancy=occ)),
        ("eager: a wrong u_f", RuntimeError, lambda: train_step_hierarchical(net_c, net_f, sgd, rays, gt, Nc, Nf, u_f=u_c, occupancy=occ)),
        ("render: grad enabled", RuntimeError, lambda: render_hierarchical(rays, net_c, net_f, Nc, Nf, occupancy=occ)),
        ("view: grad enabled", RuntimeError, lambda: render_hierarchical_view(net_c, net_f, pose, cam, Nc, Nf, occupancy=occ)),
    ]
    for what, exc, call in cases:
        state = torch.get_rng_state()
        with pytest.raises(exc):
            call()
        assert torch.equal(torch.get_rng_state(), state), what
    with torch.no_grad():
        for what, exc, call in (
                ("render: not a grid", TypeError, lambda: render_hierarchical(rays, net_c, net_f, Nc, Nf, occupancy="grid")),
                ("render: another network size", RuntimeError, lambda: render_hierarchical(rays, net_c, small, Nc, Nf, occupancy=occ)),
                ("render: Nc < 3", ValueError, lambda: render_hierarchical(rays, net_c, net_f, 2, 8, occupancy=occ)),
                ("render: a wrong u_c", RuntimeError, lambda: render_hierarchical(rays, net_c, net_f, Nc, Nf, u_c=u_f, occupancy=occ)),
                ("view: Nc + Nf > 512", ValueError, lambda: render_hierarchical_view(net_c, net_f, pose, cam, 256, 257, occupancy=occ))):
            state = torch.get_rng_state()
            with pytest.raises(exc):
                call()
            assert torch.equal(torch.get_rng_state(), state), what
    # the optimizer and the modules are still usable: a stepper that is accepted trains
    stepper = Step(net_c, net_f, opt, B, Nc, Nf, occ, (1.0, 1.0))
    before = opt.flat.clone()
    stepper.step(rays, gt, u_c=u_c, u_f=u_f)
    torch.cuda.synchronize()
    assert not torch.equal(opt.flat, before) and opt.step_count == 1


# ---- 5. inference ----------------------------------------------------------------------------------------------------------
def render_inputs(dev, oracle, synthetic, B, Nc, Nf):
    idx = torch.from_numpy(subset(B)).to(dev)
    rays = full_rays(oracle, synthetic).to(dev)[idx].contiguous()
    return rays, full_u(Nc).to(dev)[idx].contiguous(), full_u(Nf, salt=1).to(dev)[idx].contiguous()


def assert_same_pair(got, want, where):
    (gf, gc, gts), (wf, wc, wts) = got, want
    assert same(gts, wts), (where, "ts_f")
    for name, g, w in zip(NAMES, gc, wc):
        assert same(g, w), (where, "coarse", name)
    for name, g, w in zip(NAMES, gf, wf):
        assert same(g, w), (where, "fine", name)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("B", [1, 63, 1000])
def test_masked_hierarchical_render(dev, oracle, synthetic, B, precision):
    from nerf_simple_amd.utils.rendering import render_hierarchical, render_nerf, sample_pdf
    Nc, Nf = 64, 128
    net_c, net_f = make_net(dev, "structured", precision), make_net(dev, "structured", precision, seed=1)
    rays, u_c, u_f = render_inputs(dev, oracle, synthetic, B, Nc, Nf)
    with torch.no_grad():
        # an all-live grid reproduces the dense pair bit for bit in every output
        occ = all_live_grid(dev)
        dense = render_hierarchical(rays, net_c, net_f, Nc, Nf, u_c=u_c, u_f=u_f)
        got = render_hierarchical(rays, net_c, net_f, Nc, Nf, u_c=u_c, u_f=u_f, occupancy=occ)
        assert_same_pair(got, dense, (B, precision, "all-live"))
        assert occ.last_stats["coarse"]["live"] == B * Nc and occ.last_stats["fine"]["live"] == B * (Nc + Nf)
        dense = render_hierarchical(rays, net_c, net_f, Nc, Nf, device_rng=True, seed=9, ray_id0=77)
        got = render_hierarchical(rays, net_c, net_f, Nc, Nf, device_rng=True, seed=9, ray_id0=77, occupancy=occ)
        assert_same_pair(got, dense, (B, precision, "all-live, device_rng"))
        # on the ball grid: the composition of the existing entry points
        for outside in POLICIES:
            occ = ball_grid(dev, outside)
            coarse = render_nerf(rays, net_c, Nc, u=u_c, occupancy=occ)
            live_c = occ.last_stats["live"]
            assert live_c == int(model_live(rays, (u_c, tbins(Nc, dev), 0, 0, 0), Nc, outside).sum())
            ts_c = query_points(rays, u_c, tbins(Nc, dev), 0, 0, 0, Nc)[1]
            ts_f = sample_pdf(ts_c, coarse[4], Nf, u=u_f)
            fine = render_nerf(rays, net_f, Nc + Nf, ts=ts_f, occupancy=occ)
            live_f = occ.last_stats["live"]
            got = render_hierarchical(rays, net_c, net_f, Nc, Nf, u_c=u_c, u_f=u_f, occupancy=occ)
            assert_same_pair(got, (fine, coarse, ts_f), (B, precision, outside))
            st = occ.last_stats
            assert (st["coarse"]["live"], st["fine"]["live"], st["live"], st["rays"]) == (live_c, live_f, live_c + live_f, B)
            assert st["network_launches"] == (live_c > 0) + (live_f > 0)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_view_form_is_the_rays_form_after_the_clip(dev, oracle, synthetic, precision):
    from nerf_simple_amd.utils.rendering import (generate_rays, render_hierarchical, render_hierarchical_sharded,
                                                 render_hierarchical_view)
    Nc, Nf = 64, 128
    net_c, net_f = make_net(dev, "structured", precision), make_net(dev, "structured", precision, seed=1)
    pose = oracle.spherical_to_pose(4, 30, 45)
    cam = [40, 40, synthetic.focal_from_fov(40)]
    occ = ball_grid(dev, "empty")
    with torch.no_grad():
        for ray0, n in ((0, None), (37, 1000), (1599, 1)):
            nn_ = 1600 - ray0 if n is None else n
            rays = generate_rays(pose, cam, dev, ray0, nn_)
            fine, _, _ = render_hierarchical(rays, net_c, net_f, Nc, Nf, device_rng=True, seed=5, ray_id0=ray0, occupancy=occ)
            want = torch.cat([fine[0].clamp(0., 1.), fine[1][:, None]], 1)
            got = render_hierarchical_view(net_c, net_f, pose, cam, Nc, Nf, ray0=ray0, n_rays=n, device_rng=True, seed=5, occupancy=occ)
            assert got.shape == (nn_, 4) and same(got, want), (precision, ray0, n)
            assert occ.last_stats["rays"] == nn_ and occ.last_stats["coarse"]["live"] < nn_ * Nc
            assert nn_ == 1 or occ.last_stats["coarse"]["live"] > 0
        u_c, u_f = full_u(Nc)[:1600].to(dev), full_u(Nf, salt=1)[:1600].to(dev)
        rays = generate_rays(pose, cam, dev, 0, 1600)
        fine, _, _ = render_hierarchical(rays, net_c, net_f, Nc, Nf, u_c=u_c, u_f=u_f, occupancy=occ)
        got = render_hierarchical_view(net_c, net_f, pose, cam, Nc, Nf, u_c=u_c, u_f=u_f, occupancy=occ)
        assert same(got, torch.cat([fine[0].clamp(0., 1.), fine[1][:, None]], 1))
        # the sharded form hands the keyword through (one rank here)
        assert same(render_hierarchical_sharded(net_c, net_f, pose, cam, Nc, Nf, u_c=u_c, u_f=u_f, occupancy=occ), got)


def test_reference_stream_is_consumed_as_the_dense_pair_consumes_it(dev, oracle, synthetic):
    from nerf_simple_amd.utils.rendering import render_hierarchical
    Nc, Nf, B = 64, 128, 63
    net_c, net_f = make_net(dev, "structured", "fp16"), make_net(dev, "structured", "fp16", seed=1)
    rays, _, _ = render_inputs(dev, oracle, synthetic, B, Nc, Nf)
    occ = ball_grid(dev, "live")
    with torch.no_grad():
        torch.manual_seed(5)
        render_hierarchical(rays, net_c, net_f, Nc, Nf)
        after_dense = torch.get_rng_state()
        torch.manual_seed(5)
        got = render_hierarchical(rays, net_c, net_f, Nc, Nf, occupancy=occ)
        after_masked = torch.get_rng_state()
        torch.manual_seed(5)
        u_c, u_f = torch.rand(B, Nc), torch.rand(B, Nf)                     # the pair's two draws
        after_draw = torch.get_rng_state()
        want = render_hierarchical(rays, net_c, net_f, Nc, Nf, u_c=u_c.to(dev), u_f=u_f.to(dev), occupancy=occ)
    assert torch.equal(after_masked, after_dense) and torch.equal(after_masked, after_draw)
    assert_same_pair(got, want, "reference stream")


def test_fp16_overflow_demotes_both_passes_with_one_warning(dev, oracle, synthetic):
    from nerf_simple_amd.utils.rendering import render_hierarchical
    sd = {k: v.clone() for k, v in synthetic.synthetic_state_dict(0, "structured").items()}
    gain = 1e5                               # function-preserving rescaling: the first hidden activations leave fp16's range
    sd["layers_0.0.weight"] *= gain
    sd["layers_0.0.bias"] *= gain
    sd["layers_0.2.weight"] /= gain
    net_c = make_net(dev, "structured", "fp16", sd=sd)
    net_f = make_net(dev, "structured", "fp16", seed=1)
    Nc, Nf, B = 64, 128, 1000
    rays, u_c, u_f = render_inputs(dev, oracle, synthetic, B, Nc, Nf)
    occ = ball_grid(dev, "empty")
    with torch.no_grad():
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            got = render_hierarchical(rays, net_c, net_f, Nc, Nf, u_c=u_c, u_f=u_f, occupancy=occ)
        hits = [w for w in rec if "fp16 MFMA operands left their range" in str(w.message)]
        assert len(hits) == 1, [str(w.message) for w in rec]
        assert occ.last_stats["coarse"]["network_launches"] == 2 and occ.last_stats["coarse"]["live"] > 0   # fp16, then bf16
        bf = render_hierarchical(rays, net_c, net_f, Nc, Nf, u_c=u_c, u_f=u_f, precision="bf16", occupancy=occ)
        # (the bf16 call is both passes with bf16 operands: the fine network, which never overflowed, included)
    assert_same_pair(got, bf, "demoted")
    assert torch.isfinite(got[0][0]).all() and (got[0][3] > 0).any()
