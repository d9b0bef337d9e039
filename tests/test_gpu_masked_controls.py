"""The masked training controls on the GPU (csrc/masked_controls.hip, training.Controls): background,
sigma noise and distortion loss for the masked single-network steps.

Kernel level: the noise stage on live rows against nerf_amd_sigma_noise on the dense raw those rows are scattered into; the
fused head against ITS DEFINITION, the chain of the existing entry points plus the new stage under mask_C / offsets_C
(include/nerf_amd.h), bit for bit, at every capacity of occupancy_graphed_model.capacities; against the dense head on an all-live
grid; against float64 by the rules of tests/distortion_model.py.  Step level: the graphed masked steps with ``controls=`` against
the eager ones, losses bit-equal and gradients within the dW products' run-to-run tolerance; the dense equivalence of ``controls=``
and the inference renders behind a background.

Inputs and helpers: tests/test_gpu_occupancy_graphed.py's.  N in {1, 33, 64, 65, 130} (the empty sample axis, one chunk, the
chunk boundary on both sides, three chunks) x B in {37, 576} x both outside policies of the ball grid; every batch passes
occupancy_model.require_informative, and over the two policies rays with no live sample, partly live rays and fully live rays
all occur.  Every capacity is derived from the live count the CPU model gives, never typed in."""
import warnings

import numpy as np
import pytest
import torch

import background_model as BM
import distortion_model as DM
import occupancy_graphed_model as G
import occupancy_model as M
import occupancy_train_model as T
import ray_routines_model as RM
import test_gpu_occupancy_graphed as OG
from test_gpu_occupancy_graphed import ball_grid, compare_gradients, make_net, same, step_inputs, tbins, to_dev_mask

pytestmark = pytest.mark.gpu

NS = (1, 33, 64, 65, 130)
BS = (37, 576)
POLICIES = OG.POLICIES
SENTINEL = OG.SENTINEL
STD = BM.NOISE_STD
NOISE_SEED, NOISE_BASE, NOISE_OFFSET = 7, 4, 3              # the seed directly, and as base + an offset read from device memory
RID = 77                                                    # ray id of the first ray where the jitter carries none
LAM = 0.5
# NOISE x BG x DIST: the seven combinations the entry point reaches
COMBOS = [(n, b, d) for d in (False, True) for b in (False, True) for n in (False, True) if n or b or d]
_cases = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def case(dev, oracle, synthetic, mode, N, B, outside):
    """One batch: rays, targets, jitter arguments, the CPU model's live table, the mark and a random raw_live -- formed once,
    shared by the tests, never written to."""
    key = (mode, N, B, outside)
    if key not in _cases:
        gen = torch.Generator().manual_seed(1000 * N + B)
        idx = torch.from_numpy(OG.subset(B)).to(dev)
        rays = OG.full_rays(oracle, synthetic).to(dev)[idx].contiguous()
        u = OG.full_u(N).to(dev)[idx].contiguous()
        kw, ref_args, new_args = OG.jitter_args(mode, rays, u, N, dev)
        if mode != "device_rng":                              # the jitter carries no ray ids: the noise gets some of its own
            ref_args, new_args = ref_args[:4] + (RID,), new_args[:4] + (RID,)
        live = OG.model_live(rays, ref_args, N, outside)
        M.require_informative(live, N, outside)
        m = ball_grid(dev, outside).mark(rays, N, points=True, **kw)
        total = int(live.sum())
        assert m.live == total, key
        raw_live = torch.randn(total, 4, generator=gen)
        raw_live[:, 3] *= 2.0
        _cases[key] = dict(rays=rays, u=u, gt=torch.rand(B, 3, generator=gen).to(dev), bg1=torch.rand(3, generator=gen).to(dev),
                           bgB=torch.rand(B, 3, generator=gen).to(dev), ref_args=ref_args, new_args=new_args, live=live, m=m,
                           total=total, raw_live=raw_live.to(dev))
    return _cases[key]


def test_the_batches_are_informative(dev, oracle, synthetic):
    for N in NS:
        for B in BS:
            empty = partly = full = 0
            for outside in POLICIES:
                n = case(dev, oracle, synthetic, "u", N, B, outside)["live"].sum(1)        # require_informative ran in there
                empty, partly, full = empty + int((n == 0).sum()), partly + int(((n > 0) & (n < N)).sum()), full + int((n == N).sum())
            assert empty > 0 and full > 0 and (partly > 0 or N == 1), (N, B, empty, partly, full)


# ---- the entry points through ctypes -------------------------------------------------------------------------------------------
def noise_stage(dev, raw_live, out, std, seed, seed_mem, rid, mask, offsets, B, N):
    from nerf_simple_amd import _lib
    _lib.check(_lib.lib().nerf_amd_sigma_noise_masked(
        _lib.ptr(raw_live), _lib.ptr(out), std, _lib.FLAG_SEED_IN_MEMORY if seed_mem is not None else 0, seed, _lib.ptr(seed_mem),
        rid, _lib.ptr(mask), _lib.ptr(offsets), B, N, _lib.stream_ptr(dev)), "nerf_amd_sigma_noise_masked")
    return out


def dense_noise(dev, raw, std, seed, seed_mem, rid):
    from nerf_simple_amd import _lib
    B, N = raw.shape[:2]
    out = torch.full_like(raw, float("nan"))
    _lib.check(_lib.lib().nerf_amd_sigma_noise(_lib.ptr(raw), _lib.ptr(out), std, _lib.FLAG_SEED_IN_MEMORY if seed_mem is not None else 0,
                                               seed, _lib.ptr(seed_mem), rid, B, N, _lib.stream_ptr(dev)), "nerf_amd_sigma_noise")
    return out


def terms_of(combo, c, k=0, t_far=DM.TF):
    """(bg, std, coef, t_far) of a combination; the background alternates between one colour and one per ray with ``k``"""
    noise, bg, dist = combo
    B = c["rays"].shape[0]
    return ((c["bg1"] if k % 2 else c["bgB"]) if bg else None, STD if noise else 0.0,
            float(np.float32(DM.head_coef(B, LAM))) if dist else 0.0, t_far)


def head(dev, raw, rays, args, mask, offsets, gt, terms, C, B, N, pad=8):
    """-> (rgb [B, 3], loss_ray [B], the whole sentinel-prefilled d_raw buffer [C + pad, 4]); the noise seed comes as
    NOISE_BASE + an offset of NOISE_OFFSET read from device memory, as a graph node takes it"""
    from nerf_simple_amd import _lib
    jit, tb, flags, seed, rid = args
    bg, std, coef, t_far = terms
    off = torch.tensor([NOISE_OFFSET], dtype=torch.int64, device=dev)
    rgb = torch.full((B, 3), SENTINEL, dtype=torch.float32, device=dev)
    loss = torch.full((B,), SENTINEL, dtype=torch.float32, device=dev)
    buf = torch.full((C + pad, 4), SENTINEL, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().nerf_amd_volume_render_masked_mse_backward_dist(
        _lib.ptr(raw), _lib.ptr(rays), _lib.ptr(jit), _lib.ptr(tb), flags, seed, rid, _lib.ptr(mask), _lib.ptr(offsets),
        _lib.ptr(gt), _lib.ptr(bg), 0 if bg is None or bg.dim() == 1 else 3, std, _lib.FLAG_SEED_IN_MEMORY, NOISE_BASE,
        _lib.ptr(off), t_far, coef, _lib.ptr(rgb), _lib.ptr(loss), _lib.ptr(buf), C, B, N, _lib.stream_ptr(dev)),
        "nerf_amd_volume_render_masked_mse_backward_dist")
    return rgb, loss, buf


def chain(dev, raw_kept, rays, args, mask_c, offsets_c, gt, terms, B, N):
    """The head's definition, stage by stage under mask_C / offsets_C: (rgb_bg, loss_ray, d_raw of the kept rows).  coef == 0:
    the chain without the term, loss_ray all zeros."""
    from nerf_simple_amd import _lib
    lib, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    jit, tb, flags, seed, rid = args
    bg, std, coef, t_far = terms
    stride = 0 if bg is None or bg.dim() == 1 else 3
    K = raw_kept.shape[0]
    raw_n = raw_kept
    if std and K:                                                                                            # 1
        raw_n = noise_stage(dev, raw_kept, torch.full_like(raw_kept, float("nan")), std, NOISE_SEED, None, rid, mask_c, offsets_c, B, N)
    rgb, disp, acc = torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)
    w = torch.full((B, N), float("nan"), device=dev)
    hd = (ptr(raw_n) if K else None, ptr(rays), ptr(jit), ptr(tb), flags, seed, rid, ptr(mask_c), ptr(offsets_c))
    _lib.check(lib.nerf_amd_volume_render_masked(*hd, ptr(rgb), ptr(disp), None, ptr(acc), ptr(w), B, N, st), "masked compositor")  # 2
    loss, g_w = torch.zeros(B, device=dev), None
    if coef:                                                                                                 # 3
        ts = OG.query_points(rays, jit, tb, flags, seed, rid, N)[1].contiguous()
        loss, g_w = torch.full((B,), float("nan"), device=dev), torch.full((B, N), float("nan"), device=dev)
        _lib.check(lib.nerf_amd_distortion_loss(ptr(ts), ptr(w), t_far, coef, ptr(loss), ptr(g_w), B, N, st), "distortion")
    rgb_bg, g_acc = rgb, None
    if bg is not None:                                                                                       # 4
        rgb_bg = torch.empty(B, 3, device=dev)
        _lib.check(lib.nerf_amd_background_blend(ptr(rgb), ptr(acc), None, ptr(bg), stride, ptr(rgb_bg), None, B, st), "blend")
    g = BM.mse_gradient(rgb_bg, gt).contiguous()                                                             # 5
    if bg is not None:                                                                                       # 6
        g_acc = torch.empty(B, device=dev)
        _lib.check(lib.nerf_amd_background_blend_backward(ptr(g), ptr(bg), stride, ptr(g_acc), B, st), "blend backward")
    d = torch.full((K, 4), float("nan"), device=dev)
    _lib.check(lib.nerf_amd_volume_render_masked_backward(*hd, ptr(g), None, None, ptr(g_acc), ptr(g_w), ptr(d) if K else None,
                                                          B, N, st), "masked backward")                     # 7
    return rgb_bg, loss, d


# ---- 1. the noise stage ----------------------------------------------------------------------------------------------------------
def test_noise_stage_is_the_dense_stage_at_the_live_samples(dev, oracle, synthetic):
    off = torch.tensor([NOISE_OFFSET], dtype=torch.int64, device=dev)
    for N in NS:
        for B in BS:
            for outside in POLICIES:
                c = case(dev, oracle, synthetic, "u", N, B, outside)
                where = (N, B, outside)
                m, raw_live, live = c["m"], c["raw_live"], torch.from_numpy(c["live"]).to(dev)
                dense = torch.randn(B, N, 4, generator=torch.Generator().manual_seed(5)).to(dev)    # anything at the dead samples
                dense[live] = raw_live
                for rid in (0, 12345):
                    want = dense_noise(dev, dense, STD, NOISE_SEED, None, rid)[live]
                    got = noise_stage(dev, raw_live, torch.full_like(raw_live, SENTINEL), STD, NOISE_SEED, None, rid, m.mask, m.offsets, B, N)
                    assert same(got, want) and bool(torch.isfinite(got).all()), where
                    assert same(got[:, :3], raw_live[:, :3]) and not same(got[:, 3], raw_live[:, 3]), where
                    # the seed in memory: base 4 + offset 3 against 7; in place; twice
                    mem = noise_stage(dev, raw_live, torch.full_like(raw_live, SENTINEL), STD, NOISE_BASE, off, rid, m.mask, m.offsets, B, N)
                    inplace = raw_live.clone()
                    noise_stage(dev, inplace, inplace, STD, NOISE_SEED, None, rid, m.mask, m.offsets, B, N)
                    assert same(mem, want) and same(inplace, want), where
                    assert same(dense_noise(dev, dense, STD, NOISE_BASE, off, rid)[live], want), where
                other = noise_stage(dev, raw_live, torch.full_like(raw_live, SENTINEL), STD, NOISE_SEED, None, 0, m.mask, m.offsets, B, N)
                assert not same(other, got), where                                  # the ray ids matter
                # std == 0 is the identity, out of place and in place
                ident = noise_stage(dev, raw_live, torch.full_like(raw_live, SENTINEL), 0.0, NOISE_SEED, None, 3, m.mask, m.offsets, B, N)
                assert same(ident, raw_live), where
                keep = raw_live.clone()
                assert same(noise_stage(dev, keep, keep, 0.0, NOISE_SEED, None, 3, m.mask, m.offsets, B, N), raw_live), where
    # no live row: NULL buffers, nothing launched
    from nerf_simple_amd import _lib
    mask0, off0 = torch.zeros((5, 1), dtype=torch.int64, device=dev), torch.zeros(6, dtype=torch.int64, device=dev)
    assert _lib.lib().nerf_amd_sigma_noise_masked(None, None, STD, 0, 1, None, 0, _lib.ptr(mask0), _lib.ptr(off0), 5, 33,
                                                  _lib.stream_ptr(dev)) == 0


# ---- 2. the fused head is its chain ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["u", "ts", "device_rng"])
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "".join(n for n, on in zip(("noise", "Bg", "Dist"), c) if on))
def test_head_is_the_chain_under_mask_C(dev, oracle, synthetic, combo, mode):
    exact = surplus = cut = 0
    for N in NS:
        for B in BS:
            for outside in POLICIES:
                c = case(dev, oracle, synthetic, mode, N, B, outside)
                rays, gt, m, live, total, raw_live = c["rays"], c["gt"], c["m"], c["live"], c["total"], c["raw_live"]
                ray_starts = set(M.offsets(live).tolist())
                caps = G.capacities(total, B, N)
                # the capacities include exactly P', surplus rows, and (N > 1) an overflow that cuts inside a ray
                assert total in caps and any(C > total for C in caps), (N, B, outside, caps)
                assert N == 1 or any(C < total and C not in ray_starts for C in caps), (N, B, outside, caps)
                for k, C in enumerate(caps):
                    where = (combo, mode, N, B, outside, C, total)
                    # every third capacity: the last samples lie behind the far plane
                    terms = terms_of(combo, c, k, DM.TF if k % 3 else 4.0)
                    bg = terms[0]
                    kept = min(total, C)
                    kept_mask = G.mask_C(live, C)
                    mask_c, offsets_c = to_dev_mask(kept_mask, dev)
                    raw = torch.full((C, 4), float("nan"), device=dev)                # rows beyond `kept`: NaN, never read
                    raw[:kept] = raw_live[:kept]
                    rgb_ref, loss_ref, d_ref = chain(dev, raw_live[:kept].contiguous(), rays, c["ref_args"], mask_c, offsets_c, gt,
                                                     terms, B, N)
                    rgb, loss, dbuf = head(dev, raw, rays, c["new_args"], m.mask, m.offsets, gt, terms, C, B, N)
                    rgb2, loss2, dbuf2 = head(dev, raw, rays, c["new_args"], m.mask, m.offsets, gt, terms, C, B, N)
                    assert same(rgb, rgb2) and same(loss, loss2) and same(dbuf, dbuf2), where          # two runs, the same bytes
                    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(loss).all()), where
                    assert same(rgb, rgb_ref), where
                    assert same(loss, loss_ref), where
                    assert bool((dbuf[kept:C] == 0).all()) and bool((dbuf[C:] == SENTINEL).all()), where   # surplus rows; nothing beyond C
                    got = dbuf[:kept]
                    assert bool(torch.isfinite(d_ref).all()) and bool(torch.isfinite(got).all()), where
                    assert same(got, d_ref), where
                    # a ray with nothing kept: rgb = bg exactly, no weight
                    none = torch.from_numpy(kept_mask.sum(1) == 0).to(dev)
                    want_bg = torch.zeros(B, 3, device=dev) if bg is None else bg.expand(B, 3)
                    assert same(rgb[none], want_bg[none]) and not bool(loss[none].any()), where
                    if N == 1:                                                            # every output has its defined value
                        assert same(rgb, want_bg) and not bool(loss.any()) and not bool(got.any()), where
                    if not combo[2]:
                        assert not bool(loss.any()), where                                # coef == 0: all zeros
                    exact, surplus, cut = exact + (C == total), surplus + (C > total), cut + (C < total and C not in ray_starts)
    assert exact and surplus and cut


def test_no_term_is_the_plain_masked_head(dev, oracle, synthetic):
    N, B = 65, 37
    c = case(dev, oracle, synthetic, "u", N, B, "empty")
    C = c["total"] + 3
    raw = torch.full((C, 4), float("nan"), device=dev)
    raw[:c["total"]] = c["raw_live"]
    rgb, loss, dbuf = head(dev, raw, c["rays"], c["new_args"], c["m"].mask, c["m"].offsets, c["gt"], (None, 0.0, 0.0, DM.TF), C, B, N)
    rgb_p, dbuf_p = OG.fused_head(raw, c["rays"], c["new_args"], c["m"].mask, c["m"].offsets, c["gt"], C, B, N, dev)
    assert same(rgb, rgb_p) and same(dbuf, dbuf_p) and not bool(loss.any())


def test_a_dead_sample_stays_dead_whatever_the_noise(dev, oracle, synthetic):
    """std = 1e30 through the eager path: alpha and w of the dead samples are exactly 0, rays with no live sample show the
    background exactly, and the head under the same noise leaves finite zeros where nothing is kept."""
    from nerf_simple_amd.training import Controls, render_nerf_masked
    N, B = 65, 37
    c = case(dev, oracle, synthetic, "u", N, B, "empty")
    net = make_net(dev, "default")
    bg = c["bgB"]
    out = render_nerf_masked(c["rays"], net, N, ball_grid(dev, "empty"), u=c["u"], ray_id0=RID,
                             controls=Controls(background=bg, sigma_noise=1e30, noise_seed=3))
    dead = torch.from_numpy(~c["live"]).to(dev)
    assert not bool(out[2][dead].any()) and not bool(out[4][dead].any())
    assert not bool(torch.isnan(out[2]).any()) and not bool(torch.isnan(out[4]).any())
    none = torch.from_numpy(c["live"].sum(1) == 0).to(dev)
    assert bool(none.any()) and same(out[0][none], bg[none])
    C = c["total"]
    rgb, loss, dbuf = head(dev, c["raw_live"], c["rays"], c["new_args"], c["m"].mask, c["m"].offsets, c["gt"],
                           (bg, 1e30, float(np.float32(DM.head_coef(B, LAM))), DM.TF), C, B, N)
    assert same(rgb[none], bg[none]) and not bool(loss[none].any()) and not bool(torch.isnan(rgb).any())


# ---- 3. an all-live grid is the dense head ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "".join(n for n, on in zip(("noise", "Bg", "Dist"), c) if on))
def test_all_live_grid_is_the_dense_head(dev, oracle, synthetic, combo):
    from nerf_simple_amd import _lib
    B = 37
    for N in NS:
        c = case(dev, oracle, synthetic, "ts", N, B, "live")
        rays, gt = c["rays"], c["gt"]
        ts = c["new_args"][0]
        bg, std, coef, t_far = terms_of(combo, c, N)
        raw = torch.randn(B, N, 4, generator=torch.Generator().manual_seed(N)).to(dev)
        mask, offsets = to_dev_mask(np.ones((B, N), bool), dev)
        rgb, loss, dbuf = head(dev, raw.view(-1, 4), rays, c["new_args"], mask, offsets, gt, (bg, std, coef, t_far), B * N, B, N)
        rgb_d, loss_d = torch.full((B, 3), float("nan"), device=dev), torch.full((B,), float("nan"), device=dev)
        d_d = torch.full((B, N, 4), float("nan"), device=dev)
        _lib.check(_lib.lib().nerf_amd_volume_render_mse_backward_dist(
            _lib.ptr(raw), _lib.ptr(ts), _lib.ptr(rays), _lib.ptr(gt), _lib.ptr(bg), 0 if bg is None or bg.dim() == 1 else 3, std, 0,
            NOISE_SEED, None, RID, t_far, coef, _lib.ptr(rgb_d), _lib.ptr(loss_d), _lib.ptr(d_d), B, N, _lib.stream_ptr(dev)),
            "dense head")
        assert same(rgb, rgb_d) and same(loss, loss_d) and same(dbuf[:B * N], d_d.view(-1, 4)), (combo, N)
        assert bool((dbuf[B * N:] == SENTINEL).all())


# ---- 4. float64 ------------------------------------------------------------------------------------------------------------------
def test_head_against_float64(dev, oracle, synthetic):
    """d_raw_live of the all-terms head against the float64 gradient of the TOTAL loss of the same chain under the mask
    (distortion_model.head_model on the dense raw with (0, 0, 0, -inf) at the dead samples, the noise taken from the stage): the
    compositor backward's per-ray rule with the constants of tests/distortion_model.py, as tests/test_gpu_distortion.py applies
    them."""
    worst, failed = {}, []
    for N, B, outside in ((33, 37, "empty"), (65, 37, "live"), (130, 37, "empty"), (64, 576, "live")):
        c = case(dev, oracle, synthetic, "ts", N, B, outside)
        rays, gt, live, total, m = c["rays"], c["gt"], c["live"], c["total"], c["m"]
        bg = c["bgB"]
        coef = DM.head_coef(B)
        terms = (bg, STD, float(np.float32(coef)), DM.TF)
        rgb_h, loss_h, dbuf = head(dev, c["raw_live"], rays, c["new_args"], m.mask, m.offsets, gt, terms, total, B, N)
        noisy = noise_stage(dev, c["raw_live"], torch.empty_like(c["raw_live"]), STD, NOISE_SEED, None, RID, m.mask, m.offsets, B, N)
        dense = T.scatter_live(noisy.cpu(), live)
        ts = c["new_args"][0].cpu()
        cpu = (dense, ts, rays.cpu(), gt.cpu(), bg.cpu())
        want, A, rgb64, D, tol_D = DM.head_model(*cpu, float(np.float32(coef)))
        keep = np.isfinite(DM.oracle_total_grad(*cpu, coef, torch.float32)) & live[:, :, None]
        got = np.zeros((B, N, 4))
        got[live] = dbuf[:total].cpu().double().numpy()
        assert np.isfinite(got[keep]).all(), (N, B, outside)
        assert np.abs(rgb_h.cpu().double().numpy() - rgb64).max() <= 64 * BM.EPS * max(1.0, np.abs(rgb64).max()), (N, B, outside)
        r_loss = DM.ratio(loss_h.cpu().numpy(), D, tol_D)
        cond, plain = RM.ray_ratios(got, want, A, keep)
        for key, r, limit in (("conditioned", float(cond.max()), RM.bound(DM.C_REF_DIST_HEAD)),
                              ("plain", float(np.nanmax(plain, initial=0.0)), RM.bound(DM.C_REF_DIST_HEAD_PLAIN)),
                              ("loss_ray", r_loss, 1.0)):
            if key not in worst or r / limit > worst[key][0] / worst[key][1]:
                worst[key] = (r, limit, (N, B, outside))
            if not r <= limit:
                failed.append(((N, B, outside), key, r, limit))
    print("masked head vs float64: " + ", ".join(f"{k} {v[0]:.2f} of {v[1]:.1f} ({v[2]})" for k, v in worst.items()))
    assert not failed, failed


# ---- 5. the steps ----------------------------------------------------------------------------------------------------------------
def controls_of(bg, noise_seed=40):
    from nerf_simple_amd.training import Controls
    return Controls(background=bg, sigma_noise=STD, noise_seed=noise_seed, distortion=LAM)


def graphed_step(dev, kind, occ, rays, gt, u, N, C, controls, **kw):
    """one graphed masked step with lr = 0 -> (loss, {name: gradient}, the stepper)"""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedMaskedTrainStep
    net = make_net(dev, kind)
    stepper = GraphedMaskedTrainStep(net, FusedAdam(net, lr=0.0), rays.shape[0], N, occ, C, controls=controls, **kw)
    loss = stepper.step(rays.to(dev), gt.to(dev), u=None if u is None else u.to(dev)).clone()
    return loss, {k: p.grad.clone() for k, p in net.named_parameters()}, stepper


def eager_step(dev, kind, occ, rays, gt, u, N, controls, kept_mask=None, ray_id0=0):
    """the eager masked step with lr = 0; with ``kept_mask`` the autograd functions composed under mask_C"""
    from nerf_simple_amd import training
    net = make_net(dev, kind)
    rays, gt, u = rays.to(dev), gt.to(dev), u.to(dev)
    B = rays.shape[0]
    if kept_mask is None:
        opt = torch.optim.SGD(net.parameters(), lr=0.0)
        loss = training.train_step(net, opt, rays, gt, N, u=u, occupancy=occ, ray_id0=ray_id0, controls=controls)
        term = loss.distortion
    else:
        tb = tbins(N, dev)
        m = occ.mark(rays, N, u=u, points=True)
        K = int(kept_mask.sum())
        mask_c, offsets_c = to_dev_mask(kept_mask, dev)
        params = [p for _, p in net.named_parameters()]
        raw, _ = training._FusedDense.apply(net, None, None, None, 0, 0, 0, 1, m.points[:K].contiguous(), *params)
        raw = training._MaskedSigmaNoise.apply(raw.reshape(-1, 4), controls.sigma_noise, controls.noise_seed, ray_id0,
                                               (mask_c, offsets_c, B, N))
        out = training._MaskedVolumeRender.apply(raw, (rays, u, tb, 0, 0, 0, mask_c, offsets_c), B, N)
        bg, stride = (controls.background, 0) if controls.background.dim() == 1 else (controls.background, 3)
        rgb = training._Background.apply(out[0], out[3], bg.contiguous(), stride)
        ts = OG.query_points(rays, u, tb, 0, 0, 0, N)[1]
        term = training._distortion_term(out[4], ts, controls.distortion, 2, 6)
        loss = training.mse_loss(rgb, gt) + term
        loss.backward()
        loss, term = loss.detach(), term.detach()
    return loss, {k: p.grad for k, p in net.named_parameters()}, term


@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("case_", OG.STEP_CASES)
def test_graphed_step_with_controls_is_the_eager_masked_step(dev, oracle, synthetic, case_, kind):
    B, N, outside = case_
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    live = OG.model_live(rays.to(dev), (u.to(dev), tbins(N, dev), 0, 0, 0), N, outside)
    M.require_informative(live, N, outside)
    total = int(live.sum())
    occ = ball_grid(dev, outside)
    bg = torch.rand(B, 3, generator=torch.Generator().manual_seed(B)).to(dev)
    c = controls_of(bg if kind == "default" else bg[0].contiguous())
    # step 1 of the stepper draws its noise with noise_seed + 1
    want_loss, want, want_term = eager_step(dev, kind, occ, rays, gt, u, N, c.replace(noise_seed=c.noise_seed + 1), ray_id0=5)
    assert occ.last_stats["live"] == total
    plain_loss, _ = OG.eager_step(dev, kind, occ, rays, gt, u, N)
    assert not same(want_loss, plain_loss)                                                  # the terms did matter
    for C in (total, min(-(-(total + 1) // 256) * 256, B * N)):                             # exactly, and with surplus rows
        loss, grads, stepper = graphed_step(dev, kind, occ, rays, gt, u, N, C, c, ray_id0=5)
        assert stepper.counts() == {"step": 1, "samples": B * N, "live": total, "kept": total, "capacity": C}
        assert same(loss, want_loss), (case_, kind, C, float(loss), float(want_loss))
        assert same(stepper.distortion, want_term), (case_, kind, C, float(stepper.distortion), float(want_term))
        assert N == 1 or float(want_term) > 0
        compare_gradients(grads, want, (case_, kind, C))


@pytest.mark.parametrize("kind", ["default", "structured"])
@pytest.mark.parametrize("case_", [(576, 64, "empty"), (37, 65, "empty")])
def test_overflowing_step_with_controls_is_the_eager_composition_under_mask_C(dev, oracle, synthetic, case_, kind):
    B, N, outside = case_
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    live = OG.model_live(rays.to(dev), (u.to(dev), tbins(N, dev), 0, 0, 0), N, outside)
    total = int(live.sum())
    C = -(-total // 2)
    assert C not in set(M.offsets(live).tolist())                                          # the capacity cuts inside a ray
    occ = ball_grid(dev, outside)
    bg = torch.rand(B, 3, generator=torch.Generator().manual_seed(B)).to(dev)
    c = controls_of(bg if kind == "default" else bg[0].contiguous())
    c1 = c.replace(noise_seed=c.noise_seed + 1)
    want_loss, want, want_term = eager_step(dev, kind, occ, rays, gt, u, N, c1, kept_mask=G.mask_C(live, C))
    full_loss, _, _ = eager_step(dev, kind, occ, rays, gt, u, N, c1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        loss, grads, stepper = graphed_step(dev, kind, occ, rays, gt, u, N, C, c)
        assert stepper.counts() == {"step": 1, "samples": B * N, "live": total, "kept": C, "capacity": C}
    assert same(loss, want_loss), (case_, kind, float(loss), float(want_loss))
    assert same(stepper.distortion, want_term)
    assert not same(loss, full_loss)                                                       # the dropped tail did matter
    compare_gradients(grads, want, (case_, kind, C))


def test_eager_step_is_the_torch_expression_on_the_masked_render(dev, oracle, synthetic):
    """loss = mse(rgb + (1 - acc) bg, gt) + term: the blend as torch's own fp32 expression (two rounded operations per channel,
    the kernel's), the MSE and the term through the library, one fp32 add -- on the outputs of render_nerf_masked under the
    same noise, without the blend."""
    from nerf_simple_amd import training
    B, N, outside = 37, 65, "live"
    rays, gt, u = (x.to(dev) for x in step_inputs(oracle, synthetic, B, N))
    occ = ball_grid(dev, outside)
    bgB = torch.rand(B, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    for bg in (bgB, bgB[0].contiguous()):
        c = controls_of(bg)
        loss, grads, term = eager_step(dev, "default", occ, rays, gt, u, N, c, ray_id0=9)
        net = make_net(dev, "default")
        rgb, _, _, acc, w = training.render_nerf_masked(rays, net, N, occ, u=u, ray_id0=9,
                                                        controls=training.Controls(sigma_noise=c.sigma_noise, noise_seed=c.noise_seed))
        want_term = training._distortion_term(w, w.ts, LAM, 2, 6)
        want = training.mse_loss(rgb + (1 - acc)[:, None] * bg, gt) + want_term
        assert same(loss, want.detach()) and same(term, want_term.detach()), (float(loss), float(want))
        want.backward()
        compare_gradients(grads, {k: p.grad for k, p in net.named_parameters()}, "eager masked step with controls")


# ---- 6. a trajectory ---------------------------------------------------------------------------------------------------------------
def test_graphed_trajectory_with_controls(dev, oracle, synthetic):
    """8 replays with all three terms and device_rng=True against 8 eager masked steps with seed + k and noise_seed + k, losses
    and distortion terms bit-equal at every step.  lr = 0: the dW products' last bits vary from run to run (compare_gradients),
    so trained weights would not be bit-reproducible; what varies per step here is the jitter, the noise, the grid (updated in
    place behind replay 3) and the background (overwritten in place behind replay 5)."""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedMaskedTrainStep, train_step
    from nerf_simple_amd.utils import mesh
    from nerf_simple_amd.utils.occupancy import TrainingOccupancyGrid
    B, N, seed, R = 576, 64, 40, (33, 33, 33)
    rays, gt, _ = step_inputs(oracle, synthetic, B, N)
    rays, gt = rays.to(dev), gt.to(dev)
    occ = TrainingOccupancyGrid(R, OG.BOUNDS, outside="empty", device=dev)
    bg = torch.rand(B, 3, generator=torch.Generator().manual_seed(8)).to(dev)
    c = controls_of(bg, noise_seed=900)
    net, twin = make_net(dev, "structured"), make_net(dev, "structured")
    stepper = GraphedMaskedTrainStep(net, FusedAdam(net, lr=0.0), B, N, occ, 1.0, device_rng=True, seed=seed, ray_id0=11, controls=c)
    assert stepper.background.data_ptr() != bg.data_ptr() and stepper.distortion_weight == LAM and stepper.sigma_noise == STD
    opt_twin = torch.optim.SGD(twin.parameters(), lr=0.0)
    losses, lives = [], []
    for k in range(1, 9):
        if k == 4:
            sigma = mesh.density_grid(net, R, OG.BOUNDS).cpu().numpy()
            occ.update(net, float(np.percentile(sigma, 90)), decay=0.5, dilate=1)
        if k == 6:
            bg = 1.0 - bg
            stepper.background.copy_(bg)                                                   # in place: the next replay reads it
        loss = stepper.step(rays, gt).clone()
        want = train_step(twin, opt_twin, rays, gt, N, device_rng=True, seed=seed + k, ray_id0=11, occupancy=occ,
                          controls=c.replace(noise_seed=c.noise_seed + k, background=bg))
        assert same(loss, want), (k, float(loss), float(want))
        assert same(stepper.distortion, want.distortion), k
        losses.append(float(loss))
        lives.append(occ.last_stats["live"])
    assert stepper.counts()["live"] == lives[-1] and stepper.overflow_steps == 0
    assert lives[3] < lives[2] and len(set(losses)) == 8


# ---- 7. the masked guided stepper --------------------------------------------------------------------------------------------------
def test_graphed_masked_guided_step_with_controls(dev, oracle, synthetic):
    import occupancy_hierarchical_model as H
    from nerf_simple_amd import training
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.utils.proposal import ProposalVolume
    B, Nc, Nf, seed, rid = 37, 32, 32, 400, 7
    rays, gt, _, _ = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, B, Nc, Nf))
    net, twin, structured = make_net(dev, "default"), make_net(dev, "default"), make_net(dev, "structured")
    prop = ProposalVolume(17, OG.BOUNDS, device=dev).update(structured)
    occ = ball_grid(dev, "empty")
    c = controls_of(torch.rand(B, 3, generator=torch.Generator().manual_seed(2)).to(dev))
    stepper = training.GraphedMaskedGuidedTrainStep(net, FusedAdam(net, lr=0.0), B, Nc, Nf, prop, occ, 1.0, device_rng=True, seed=seed,
                                                    ray_id0=rid, controls=c)
    opt_twin = FusedAdam(twin, lr=0.0)
    for k in (1, 2):
        loss = stepper.step(rays, gt).clone()
        want = training.train_step_guided(twin, opt_twin, rays, gt, Nc, Nf, prop, device_rng=True, seed=seed + k, ray_id0=rid,
                                          occupancy=occ, controls=c.replace(noise_seed=c.noise_seed + k))
        live = occ.last_stats["live"]
        assert 0 < live < B * (Nc + Nf) and stepper.counts()["live"] == live
        assert same(loss, want), (k, float(loss), float(want))
        assert same(stepper.distortion, want.distortion) and float(want.distortion) > 0, k
        assert same(stepper.ts_f, want.ts), k
        compare_gradients({n: p.grad for n, p in net.named_parameters()}, {n: p.grad for n, p in twin.named_parameters()}, k)
    plain = training.train_step_guided(twin, opt_twin, rays, gt, Nc, Nf, prop, device_rng=True, seed=seed + 2, ray_id0=rid, occupancy=occ)
    assert not same(plain, want)


# ---- 8. an all-dead batch ----------------------------------------------------------------------------------------------------------
def test_all_dead_batch_with_controls(dev, oracle, synthetic):
    from nerf_simple_amd import _lib
    B, N = 576, 64
    rays, gt, u = step_inputs(oracle, synthetic, B, N)
    away = torch.cat([rays[:, :3], -rays[:, 3:]], 1).contiguous()       # the camera looks away from the grid
    assert not OG.model_live(away.to(dev), (u.to(dev), tbins(N, dev), 0, 0, 0), N, "empty").any()
    bg = torch.rand(B, 3, generator=torch.Generator().manual_seed(4)).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                   # no overflow is reported
        loss, grads, stepper = graphed_step(dev, "default", ball_grid(dev, "empty"), away, gt, u, N, 0.25, controls_of(bg))
        assert stepper.counts() == {"step": 1, "samples": B * N, "live": 0, "kept": 0, "capacity": B * N // 4}
    want = torch.empty((), device=dev)
    _lib.check(_lib.lib().nerf_amd_mse_loss(_lib.ptr(bg), _lib.ptr(gt.to(dev)), _lib.ptr(want), None, B * 3, _lib.stream_ptr(dev)), "mse")
    assert same(loss, want) and same(stepper.rgb, bg) and float(stepper.distortion) == 0.0, (float(loss), float(want))
    for k, g in grads.items():
        assert (g == 0).all(), k
    eager, egrads, _ = eager_step(dev, "default", ball_grid(dev, "empty"), away, gt, u, N, controls_of(bg, 41))
    assert same(eager, want) and all(bool((g == 0).all()) for g in egrads.values())


# ---- 9. the dense equivalence and the inference renders ----------------------------------------------------------------------------
def test_dense_steps_take_controls_as_their_flat_keywords(dev, oracle, synthetic):
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import Controls, GraphedTrainStep, train_step
    B, N = 37, 65
    rays, gt, u = (x.to(dev) for x in step_inputs(oracle, synthetic, B, N))
    bg = torch.rand(B, 3, generator=torch.Generator().manual_seed(6)).to(dev)
    flat = dict(background=bg, sigma_noise=STD, noise_seed=12, distortion=LAM)
    runs = []
    for kw in (flat, dict(controls=Controls(**flat))):
        net = make_net(dev, "default")
        loss = train_step(net, torch.optim.SGD(net.parameters(), lr=0.0), rays, gt, N, u=u, ray_id0=3, **kw)
        net_g = make_net(dev, "default")
        stepper = GraphedTrainStep(net_g, FusedAdam(net_g, lr=0.0), B, N, ray_id0=3, **kw)
        runs.append((loss, loss.distortion, stepper.step(rays, gt, u=u).clone(), stepper.distortion.clone(), stepper.rgb.clone()))
    for a, b in zip(*runs):
        assert same(a, b)
    assert float(runs[0][1]) > 0


def test_inference_renders_blend_behind_the_masked_render(dev, oracle, synthetic):
    from nerf_simple_amd.training import Controls
    from nerf_simple_amd.utils import metrics  # noqa: F401  (evaluate's pass-through is render_view's keyword)
    from nerf_simple_amd.utils.rendering import render_nerf, render_view
    N, B = 65, 37
    c = case(dev, oracle, synthetic, "u", N, B, "empty")
    occ, net = ball_grid(dev, "empty"), make_net(dev, "structured")
    with torch.no_grad():
        for bg in (c["bgB"], c["bg1"]):
            plain = render_nerf(c["rays"], net, N, u=c["u"], occupancy=occ)
            got = render_nerf(c["rays"], net, N, u=c["u"], occupancy=occ, controls=Controls(background=bg))
            assert same(got[0], plain[0] + (1 - plain[3])[:, None] * bg) and not same(got[0], plain[0])
            assert all(same(a, b) for a, b in zip(got[1:], plain[1:]))
        # a view: the clip behind the blend
        pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, 30, 45))).float()
        cam = [10, 10, synthetic.focal_from_fov(10)]
        from nerf_simple_amd.utils.rendering import generate_rays
        rays = generate_rays(pose, cam, dev)
        u = torch.rand(100, N, generator=torch.Generator().manual_seed(1)).to(dev)
        bg = torch.tensor([1.0, 0.5, 0.0], device=dev)
        plain = render_nerf(rays, net, N, u=u, occupancy=occ)
        px = render_view(net, pose, cam, N=N, u=u, occupancy=occ, controls=Controls(background=bg))
        assert same(px[:, :3], torch.clip(plain[0] + (1 - plain[3])[:, None] * bg, 0., 1.)) and same(px[:, 3], plain[1])
        assert not same(px, render_view(net, pose, cam, N=N, u=u, occupancy=occ))
