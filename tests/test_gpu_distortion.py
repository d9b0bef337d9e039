"""The distortion loss on the GPU.

  stage      nerf_amd_distortion_loss against the float64 model (tests/distortion_model.py) on every committed case, within
             bound(C_REF_DIST_GW) / bound(C_REF_DIST_LOSS) of the model's units; N == 1, B == 0, sentinel padding
  head       nerf_amd_volume_render_mse_backward_dist == its chain bit for bit (alone, behind either background, with noise,
             with both, coef == 0 against the _bg head), against float64 by the compositor backward's per-ray rule, and a
             descent check that rests on the float64 D alone
  Python     train_step / train_step_guided (bf16 and fp32), GraphedTrainStep / GraphedGuidedTrainStep
"""
import numpy as np
import pytest
import torch

import background_model as BM
import distortion_model as DM
import ray_routines_model as M
from test_gpu_background import RAY0, SEED, blend, blend_backward, fresh, noise, weights
from test_gpu_guided import BOUNDS
from test_gpu_occupancy_graphed import compare_gradients

pytestmark = pytest.mark.gpu
LAM = 0.5                     # the head's cases (random raw: spread weights)
LAM_STEP = 16.0               # the steps: the scene's weights are compact, D / (tf - tn) is of the order 1e-3 per ray
PAD, SENTINEL = 64, -12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def bits(t_):
    return t_.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- the entry points through ctypes ------------------------------------------------------------------------------------------
def stage(dev, ts, w, t_far, coef, want_loss=True, want_grad=True):
    """(loss_ray [B], g_w [B,N]) on the device, pre-filled with NaN: an unwritten element shows."""
    from nerf_simple_amd import _lib
    B, N = ts.shape
    loss = torch.full((B,), float("nan"), device=dev) if want_loss else None
    g_w = torch.full((B, N), float("nan"), device=dev) if want_grad else None
    _lib.check(_lib.lib().nerf_amd_distortion_loss(_lib.ptr(ts), _lib.ptr(w), t_far, coef, _lib.ptr(loss), _lib.ptr(g_w), B, N,
                                                   _lib.stream_ptr(dev)), "nerf_amd_distortion_loss")
    return loss, g_w


def head(dev, raw, ts, rays, target, bg, std, coef, t_far=DM.TF, seed=SEED, ray_id0=RAY0):
    from nerf_simple_amd import _lib
    B, N = ts.shape
    rgb, loss = torch.full((B, 3), float("nan"), device=dev), torch.full((B,), float("nan"), device=dev)
    d_raw = torch.full((B, N, 4), float("nan"), device=dev)
    _lib.check(_lib.lib().nerf_amd_volume_render_mse_backward_dist(
        _lib.ptr(raw), _lib.ptr(ts), _lib.ptr(rays), _lib.ptr(target), _lib.ptr(bg), 0 if bg is None or bg.dim() == 1 else 3, std, 0,
        seed, None, ray_id0, t_far, coef, _lib.ptr(rgb), _lib.ptr(loss), _lib.ptr(d_raw), B, N, _lib.stream_ptr(dev)),
        "nerf_amd_volume_render_mse_backward_dist")
    return rgb, loss, d_raw


def chain(dev, raw, ts, rays, target, bg, std, coef, t_far=DM.TF, seed=SEED, ray_id0=RAY0):
    """The head's definition, stage by stage: (rgb_bg, loss_ray, d_raw)."""
    from nerf_simple_amd import _lib
    lib, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    B, N = ts.shape
    raw_n = noise(dev, raw, std, seed, ray_id0) if std else raw                                              # 1
    rgb, disp, acc = torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)
    w = torch.full((B, N), float("nan"), device=dev)
    _lib.check(lib.nerf_amd_volume_render_rays(ptr(raw_n), ptr(ts), ptr(rays), ptr(rgb), ptr(disp), None, ptr(acc), ptr(w), B, N, st),
               "nerf_amd_volume_render_rays")                                                              # 2
    loss, g_w = stage(dev, ts, w, t_far, coef)                                                               # 3
    rgb_bg = rgb if bg is None else blend(dev, rgb, acc, None, bg, pixels=False)[0]                          # 4
    g = BM.mse_gradient(rgb_bg, target).contiguous()                                                         # 5
    g_acc = None if bg is None else blend_backward(dev, g, bg)                                               # 6
    d_raw = torch.full((B, N, 4), float("nan"), device=dev)
    _lib.check(lib.nerf_amd_volume_render_rays_backward(ptr(raw_n), ptr(ts), ptr(rays), ptr(g), None, None, ptr(g_acc), ptr(g_w),
                                                        ptr(d_raw), B, N, st), "nerf_amd_volume_render_rays_backward")      # 7
    return rgb_bg, loss, d_raw


_inputs = {}


def head_inputs(dev, case):
    """A head case's inputs on the device: formed once, shared, never written to."""
    if case.id not in _inputs:
        _inputs[case.id] = tuple(x.to(dev).contiguous() for x in BM.head_inputs(case))
    return _inputs[case.id]


# ---- the stage ----------------------------------------------------------------------------------------------------------------
def test_stage_against_the_model(dev):
    cases = DM.cases()
    assert {c.N for c in cases} == set(DM.DIST_N) and {c.B for c in cases} == set(DM.DIST_B)
    lim_g, lim_D = M.bound(DM.C_REF_DIST_GW), M.bound(DM.C_REF_DIST_LOSS)
    worst_g = worst_D = (0.0, None)
    failed = []
    for k, case in enumerate(cases):
        ts, w, t_far = DM.inputs(case)
        coef = (1.0, 0.25, 1.0 / (case.B * 4.0))[k % 3]
        loss, g_w = stage(dev, ts.to(dev), w.to(dev), t_far, coef)
        c32 = float(np.float32(coef))
        D, g, unit_D, unit_g = DM.model(ts, w, t_far, c32)
        r_D, r_g = DM.ratio(loss.cpu().numpy(), D, unit_D), DM.ratio(g_w.cpu().numpy(), g, unit_g)
        worst_g, worst_D = max(worst_g, (r_g, case.id)), max(worst_D, (r_D, case.id))
        if not (r_g <= lim_g and r_D <= lim_D):
            failed.append((case.id, r_g, r_D))
        if case.weights == "zero":
            assert not bool(loss.any()) and not bool(g_w.any()), case.id
    print(f"stage vs float64: gradient {worst_g[0]:.2f} of {lim_g:.1f} units ({worst_g[1]}), loss {worst_D[0]:.2f} of {lim_D:.2f} ({worst_D[1]})")
    assert not failed, failed


def test_stage_edges_and_padding(dev):
    from nerf_simple_amd import _lib
    # N == 1: the reference's empty sample axis; B == 0: nothing is launched, nothing is looked at
    loss, g_w = stage(dev, torch.rand(5, 1, device=dev) + 2, torch.rand(5, 1, device=dev), 6.0, 0.25)
    assert not bool(loss.any()) and not bool(g_w.any()) and bool(torch.isfinite(loss).all())
    assert _lib.lib().nerf_amd_distortion_loss(None, None, 6.0, 0.25, None, None, 0, 64, _lib.stream_ptr(dev)) == 0
    # either output alone is the same bits
    case = next(c for c in DM.cases() if c.N == 129 and c.B == 5 and c.positions == "merged" and c.weights == "rendered")
    ts, w, t_far = (x.to(dev) if torch.is_tensor(x) else x for x in DM.inputs(case))
    both = stage(dev, ts, w, t_far, 0.25)
    assert same(stage(dev, ts, w, t_far, 0.25, want_grad=False)[0], both[0])
    assert same(stage(dev, ts, w, t_far, 0.25, want_loss=False)[1], both[1])
    # a NaN weight stays inside its ray
    wn = w.clone()
    wn[2, 70] = float("nan")
    ln, gn = stage(dev, ts, wn, t_far, 0.25)
    keep = torch.tensor([0, 1, 3, 4], device=dev)
    assert same(ln[keep], both[0][keep]) and same(gn[keep], both[1][keep]) and bool(torch.isnan(ln[2]))
    # sentinel padding: exactly B and B N elements are written
    B, N = ts.shape
    lbuf, gbuf = torch.full((B + 2 * PAD,), SENTINEL, device=dev), torch.full((B * N + 2 * PAD,), SENTINEL, device=dev)
    _lib.check(_lib.lib().nerf_amd_distortion_loss(_lib.ptr(ts), _lib.ptr(w), t_far, 0.25, _lib.ptr(lbuf[PAD:]), _lib.ptr(gbuf[PAD:]), B, N,
                                                   _lib.stream_ptr(dev)), "nerf_amd_distortion_loss")
    for buf, ref in ((lbuf, both[0]), (gbuf, both[1])):
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())
        assert same(buf[PAD:-PAD], ref.reshape(-1))
    # nerf_amd_sum_f32: a fixed order, against float64
    x = torch.rand(4099, device=dev) - 0.25
    out = torch.full((3,), SENTINEL, device=dev)
    for _ in range(2):
        _lib.check(_lib.lib().nerf_amd_sum_f32(_lib.ptr(x), _lib.ptr(out[1:]), x.numel(), _lib.stream_ptr(dev)), "nerf_amd_sum_f32")
        assert float(out[0]) == SENTINEL and float(out[2]) == SENTINEL
        assert abs(float(out[1]) - float(x.double().sum())) <= 16 * DM.EPS * float(x.double().abs().sum())
        first = out[1].clone() if _ == 0 else first
    assert same(out[1], first)


# ---- the head is its chain ----------------------------------------------------------------------------------------------------
HEAD_MODES = ("neither", "bg1", "bgB", "noise", "both", "coef0")


@pytest.mark.parametrize("mode", HEAD_MODES)
def test_head_is_the_chain(dev, mode):
    """torch.equal on rgb, loss_ray and d_raw (all pre-filled with NaN) at N in {2, 63, 64, 65, 128, 129, 512} x B in {1, 5, 37}
    and at N == 1; with coef == 0 also against nerf_amd_volume_render_mse_backward_bg, loss_ray all zeros."""
    from test_gpu_background import head as bg_head
    cases = BM.head_cases()
    for k, case in enumerate(cases):
        raw, ts, rays, target, bg1, bgB = head_inputs(dev, case)
        bg, std = BM.mode_controls("both" if mode == "coef0" else mode, bg1, bgB)
        coef = 0.0 if mode == "coef0" else DM.head_coef(case.B, LAM)
        t_far = DM.TF if k % 3 else float(ts[:, -1].min()) - 0.125          # every third case: last samples behind the far plane
        got, want = head(dev, raw, ts, rays, target, bg, std, coef, t_far), chain(dev, raw, ts, rays, target, bg, std, coef, t_far)
        for name, a, b in zip(("rgb", "loss_ray", "d_raw"), got, want):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (case.id, name)
        if mode == "coef0":
            rgb_b, d_b = bg_head(dev, raw, ts, rays, target, bg, std)
            assert torch.equal(got[0], rgb_b) and torch.equal(got[2], d_b) and not bool(got[1].any()), case.id
    for B in (1, 5):                                              # N == 1: rgb_bg = bg exactly, no weight, D = 0, d_raw = 0
        g = torch.Generator().manual_seed(B)
        raw, ts, rays = torch.randn(B, 1, 4, generator=g), torch.rand(B, 1, generator=g) * 4 + 2, torch.randn(B, 6, generator=g)
        target, bg1, bgB = torch.rand(B, 3, generator=g), torch.rand(3, generator=g), torch.rand(B, 3, generator=g)
        raw, ts, rays, target, bg1, bgB = (x.to(dev) for x in (raw, ts, rays, target, bg1, bgB))
        bg, std = BM.mode_controls("both" if mode == "coef0" else mode, bg1, bgB)
        got = head(dev, raw, ts, rays, target, bg, std, 0.125)
        want = chain(dev, raw, ts, rays, target, bg, std, 0.125)
        assert all(torch.equal(a, b) for a, b in zip(got, want)) and not bool(got[1].any()) and not bool(got[2].any())
        assert torch.equal(got[0], torch.zeros(B, 3, device=dev) if bg is None else bg.expand(B, 3))


def test_head_padding(dev):
    """rgb, loss_ray and d_raw inside sentinel padding: exactly their elements are written."""
    from nerf_simple_amd import _lib
    case = next(c for c in BM.head_cases() if c.N == 65 and c.B == 5)
    raw, ts, rays, target, bg1, bgB = head_inputs(dev, case)
    B, N = ts.shape
    coef = DM.head_coef(B, LAM)
    want = head(dev, raw, ts, rays, target, bgB, 0.5, coef)
    bufs = [torch.full((n + 2 * PAD,), SENTINEL, device=dev) for n in (B * 3, B, B * N * 4)]
    _lib.check(_lib.lib().nerf_amd_volume_render_mse_backward_dist(
        _lib.ptr(raw), _lib.ptr(ts), _lib.ptr(rays), _lib.ptr(target), _lib.ptr(bgB), 3, 0.5, 0, SEED, None, RAY0, DM.TF, coef,
        _lib.ptr(bufs[0][PAD:]), _lib.ptr(bufs[1][PAD:]), _lib.ptr(bufs[2][PAD:]), B, N, _lib.stream_ptr(dev)), "head")
    for buf, ref in zip(bufs, want):
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all()) and same(buf[PAD:-PAD], ref.reshape(-1))


def test_head_against_float64(dev):
    """float64 gradient of the TOTAL loss through ray_routines_model.model_backward with g_rgb, g_acc and g_w formed from the
    float64 forward; the compositor backward's per-ray rule (ray_ratios, bound = 2 c + 4) with the constants
    distortion_model.py measures from the reference's own fp32 evaluation of the same total loss."""
    worst, failed = {}, []
    for case, mode in DM.head_cases():
        raw, ts, rays, target, bg1, bgB = head_inputs(dev, case)
        bg = BM.mode_controls(mode, bg1, bgB)[0]
        coef = DM.head_coef(case.B)
        rgb_h, loss_h, d_h = head(dev, raw, ts, rays, target, bg, 0.0, coef)
        cpu = [None if x is None else x.cpu() for x in (raw, ts, rays, target, bg)]
        want, A, rgb64, D, tol_D = DM.head_model(*cpu, float(np.float32(coef)))
        keep = np.isfinite(DM.oracle_total_grad(*cpu, coef, torch.float32))
        got = d_h.cpu().numpy()
        assert np.isfinite(got[keep]).all(), case.id
        assert np.abs(rgb_h.cpu().double().numpy() - rgb64).max() <= 64 * BM.EPS * max(1.0, np.abs(rgb64).max()), case.id
        r_loss = DM.ratio(loss_h.cpu().numpy(), D, tol_D)
        cond, plain = M.ray_ratios(got, want, A, keep)
        for key, r, limit in (("conditioned", float(cond.max()), M.bound(DM.C_REF_DIST_HEAD)),
                              ("plain", float(np.nanmax(plain, initial=0.0)), M.bound(DM.C_REF_DIST_HEAD_PLAIN)),
                              ("loss_ray", r_loss, 1.0)):
            if key not in worst or r / limit > worst[key][0] / worst[key][1]:
                worst[key] = (r, limit, case.id)
            if not r <= limit:
                failed.append((case.id, key, r, limit))
    print("head vs float64: " + ", ".join(f"{k} {v[0]:.2f} of {v[1]:.1f} ({v[2]})" for k, v in worst.items()))
    assert not failed, failed


def test_descent_on_the_float64_loss(dev):
    """The GPU's d_raw of the distortion term alone (compositor -> nerf_amd_distortion_loss -> compositor backward with g_w only):
    D evaluated in float64 on the CPU at raw - eta d_raw lies below D(raw).  Rests on the model's D alone, not on any gradient
    of the oracle.  eta: the largest step moves a raw density by 0.05."""
    from nerf_simple_amd import _lib
    lib, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    B, N = 37, 64
    g = torch.Generator().manual_seed(64037)
    raw = torch.randn(B, N, 4, generator=g)
    raw[..., 3] = 2.0 * raw[..., 3] - 2.0
    ts = DM.O.sample_ts(torch.rand(B, N, generator=g), DM.TN, DM.TF).contiguous()
    rays = torch.cat([torch.randn(B, 3, generator=g), torch.randn(B, 3, generator=g)], dim=1)
    coef = DM.head_coef(B)
    raw_d, ts_d, rays_d = raw.to(dev), ts.to(dev), rays.to(dev)
    rgb, disp, acc, w = torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, N, device=dev)
    _lib.check(lib.nerf_amd_volume_render_rays(ptr(raw_d), ptr(ts_d), ptr(rays_d), ptr(rgb), ptr(disp), None, ptr(acc), ptr(w), B, N, st), "render")
    _, g_w = stage(dev, ts_d, w, DM.TF, coef)
    d_raw = torch.full((B, N, 4), float("nan"), device=dev)
    _lib.check(lib.nerf_amd_volume_render_rays_backward(ptr(raw_d), ptr(ts_d), ptr(rays_d), None, None, None, None, ptr(g_w), ptr(d_raw),
                                                        B, N, st), "backward")
    d_raw = d_raw.cpu()
    assert bool(torch.isfinite(d_raw).all()) and not bool(d_raw[..., :3].any()) and bool(d_raw[..., 3].any())

    def D64(r):
        fw = M.forward64(r, ts, BM.unit_dirs(rays))
        return DM.model(ts, fw["w"], DM.TF, coef)[0]

    eta = 0.05 / float(d_raw.abs().max())
    before, after = D64(raw.double()), D64(raw.double() - eta * d_raw.double())
    print(f"descent: sum D {before.sum():.6e} -> {after.sum():.6e}; {int((after < before).sum())} of {B} rays fall")
    assert after.sum() < before.sum()


# ---- the eager steps ----------------------------------------------------------------------------------------------------------
def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def scene(dev, golden, synthetic):
    g = golden("train.npz")
    gen = torch.Generator().manual_seed(23)
    B = g["rays"].shape[0]
    return dict(rays=t(g["rays"]).to(dev), gt=t(g["gt"]).to(dev), u=t(g["u"]).to(dev), N=int(g["N"]), B=B,
                bg1=torch.rand(3, generator=gen).to(dev), bgB=torch.rand(B, 3, generator=gen).to(dev))


def _grads(net):
    return {k: p.grad.clone() for k, p in net.named_parameters()}


def _eager(dev, synthetic, scene, precision="bf16", **kw):
    from nerf_simple_amd.training import train_step
    net = fresh(dev, synthetic, precision)
    loss = train_step(net, torch.optim.SGD(net.parameters(), lr=0.0), scene["rays"], scene["gt"], scene["N"], **kw)
    return loss, _grads(net), net


def test_train_step_bf16(dev, scene, synthetic):
    """distortion=0.0 is the call without it (the loss bit for bit; the dW products sum with float atomics, so two identical
    calls agree to compare_gradients only).  With the term: the loss against the float64 total on the training forward's own
    raw, the gradients against the same composition built by hand from the public pieces, alone and behind both controls."""
    from nerf_simple_amd import training
    from nerf_simple_amd.utils.controls import Resolved
    from nerf_simple_amd.utils.rendering import _tbins
    rays, gt, u, N, B = (scene[k] for k in ("rays", "gt", "u", "N", "B"))
    la, ga, _ = _eager(dev, synthetic, scene, u=u)
    lb, gb, _ = _eager(dev, synthetic, scene, u=u, distortion=0.0)
    assert same(la, lb) and not hasattr(lb, "distortion")
    compare_gradients(gb, ga, "distortion=0.0")
    for controls in (None, Resolved(scene["bgB"], 3, 0.5, 77, RAY0, 0.0)):
        kw = {} if controls is None else dict(background=controls[0], sigma_noise=controls[2], noise_seed=controls[3])
        lc, gc, _ = _eager(dev, synthetic, scene, u=u, distortion=LAM_STEP, ray_id0=RAY0, **kw)
        net = fresh(dev, synthetic)
        params = [p for _, p in net.named_parameters()]
        raw, ts = training._FusedDense.apply(net, rays, u, _tbins(2, 6, N, dev), 0, 0, 0, N, None, *params)
        out = training.composite_with_controls(raw, ts, rays, True, controls)
        per_ray = training.distortion_loss(out[4], ts)
        assert per_ray.shape == (B,) and bool((per_ray > 0).all())
        want = training.mse_loss(out[0], gt) + (LAM_STEP / B) * per_ray.sum()
        want.backward()
        want = want.detach()
        assert abs(float(lc) - float(want)) <= 1e-6 * float(want) and (controls is not None or float(lc) > float(la))
        assert abs(float(lc.distortion) - LAM_STEP / B * float(per_ray.detach().sum())) <= 1e-6 * float(lc.distortion)
        compare_gradients(gc, _grads(net), ("distortion", controls is not None))
        if controls is None:
            total = DM.total_loss(raw.detach().double().cpu(), ts.cpu(), rays.cpu(), gt.cpu(), None, DM.head_coef(B, LAM_STEP))
            print(f"bf16 step: loss {float(lc):.8f}, float64 total {float(total):.8f}, term {float(lc.distortion):.6f}")
            # 1e-6 of the total as the existing step tests hold a loss, + the term's own derived allowance per ray
            tol_D = DM.head_model(raw.detach().cpu(), ts.cpu(), rays.cpu(), gt.cpu(), None, DM.head_coef(B, LAM_STEP))[4]
            assert abs(float(lc) - float(total)) <= 1e-6 * float(total) + float(tol_D.sum())
            assert float(lc.distortion) > 0                                      # the scene's weights are spread: the term is there


def test_train_step_fp32_against_float64(dev, scene, synthetic, oracle):
    """precision='fp32' with the term behind a background, held to the float64 oracle as tests/test_gpu_training.py holds the
    fp32 step: the loss to 1e-6, every gradient tensor within 3x the distance of the reference's own fp32 evaluation (+ 3e-6).
    distortion=0.0 on this path is the call without it: the loss bit for bit, the gradients to compare_gradients (the fp32
    layers' weight gradients sum with float atomics too)."""
    rays, gt, u, N, B = (scene[k] for k in ("rays", "gt", "u", "N", "B"))
    bg = scene["bg1"]
    la, ga, _ = _eager(dev, synthetic, scene, "fp32", u=u, background=bg)
    lb, gb, _ = _eager(dev, synthetic, scene, "fp32", u=u, background=bg, distortion=0.0)
    assert same(la, lb)
    compare_gradients(gb, ga, "fp32 distortion=0.0")
    loss, _, net = _eager(dev, synthetic, scene, "fp32", u=u, background=bg, distortion=LAM_STEP)
    coef = DM.head_coef(B, LAM_STEP)

    def step(dtype):
        sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in weights(synthetic).items()}
        ts = oracle.sample_ts(u.cpu().to(dtype), 2, 6)
        q, dn = oracle.query_points(rays.cpu().to(dtype), ts)
        out = oracle.nerf_forward(sd, q).reshape(B, N, 4)
        rgb, _, _, acc, w = oracle.volume_render(out, ts, dn)
        l_ = torch.mean((rgb + (1 - acc)[:, None] * bg.cpu().to(dtype) - gt.cpu().to(dtype)) ** 2) + coef * DM.direct(ts, w, DM.TF).sum()
        l_.backward()
        return float(l_.detach()), {k: p.grad.double().numpy() for k, p in sd.items()}

    loss64, g64 = step(torch.float64)
    _, g32 = step(torch.float32)
    assert abs(float(loss) - loss64) <= 1e-6 * loss64, (float(loss), loss64)

    def rel_l2(a, b):
        return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))

    for k, p in net.named_parameters():
        ours, theirs = rel_l2(p.grad.double().cpu().numpy(), g64[k]), rel_l2(g32[k], g64[k])
        assert ours <= 3 * theirs + 3e-6, (k, ours, theirs)


def _guided_scene(dev, oracle, synthetic, B, Nc, Nf):
    import occupancy_hierarchical_model as H
    from nerf_simple_amd.utils.proposal import ProposalVolume
    rays, gt, u_c, u_f = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, B, Nc, Nf))
    prop = ProposalVolume(17, BOUNDS, device=dev)
    prop.update(fresh(dev, synthetic))
    return rays, gt, u_c, u_f, prop


def test_train_step_guided(dev, oracle, synthetic):
    """train_step_guided(distortion=) at (16 + 16): 0.0 is the call without it; with the term, the loss against the float64 total
    on the forward's own raw and the gradients against the composition by hand on the same guided positions."""
    from nerf_simple_amd import _lib, training
    from nerf_simple_amd.optim import FusedAdam
    B, Nc, Nf = 37, 16, 16
    rays, gt, u_c, u_f, prop = _guided_scene(dev, oracle, synthetic, B, Nc, Nf)
    out = []
    for kw in ({}, dict(distortion=0.0), dict(distortion=LAM_STEP)):
        net = fresh(dev, synthetic)
        loss = training.train_step_guided(net, FusedAdam(net, lr=0.0), rays, gt, Nc, Nf, prop, u_c=u_c, u_f=u_f, **kw)
        out.append((loss, _grads(net)))
    assert same(out[0][0], out[1][0]) and same(out[0][0].ts, out[2][0].ts)
    compare_gradients(out[1][1], out[0][1], "guided distortion=0.0")
    loss, ts = out[2][0], out[2][0].ts
    net = fresh(dev, synthetic)
    outs, _ = training._render_train_with_ts(rays, net, Nc + Nf, 2, 6, ts, _lib.FLAG_TS_GIVEN, "bf16", 0, 0)
    want = training.mse_loss(outs[0], gt) + (LAM_STEP / B) * training.distortion_loss(outs[4], ts).sum()
    want.backward()
    want = want.detach()
    assert abs(float(loss) - float(want)) <= 1e-6 * float(want) and float(loss) > float(out[0][0])
    compare_gradients(out[2][1], _grads(net), "guided distortion")
    params = [p for _, p in net.named_parameters()]
    with torch.no_grad():
        raw, _ = training._FusedDense.apply(net, rays, ts, None, _lib.FLAG_TS_GIVEN, 0, 0, Nc + Nf, None, *params)
    total = DM.total_loss(raw.double().cpu(), ts.cpu(), rays.cpu(), gt.cpu(), None, DM.head_coef(B, LAM_STEP))
    print(f"guided step: loss {float(loss):.8f}, float64 total {float(total):.8f}, term {float(loss.distortion):.6f}")
    tol_D = DM.head_model(raw.cpu(), ts.cpu(), rays.cpu(), gt.cpu(), None, DM.head_coef(B, LAM_STEP))[4]
    assert abs(float(loss) - float(total)) <= 1e-6 * float(total) + float(tol_D.sum())


# ---- the graphed steps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "controls", "e4m3"])
def test_graphed_step(dev, oracle, synthetic, variant):
    """GraphedTrainStep(distortion=) at 256 x 16, learning rate 0, three replays: step() and stepper.distortion are the eager
    train_step(..., seed=seed + k, noise_seed=noise_seed + k) bit for bit; lambda is read-only."""
    import occupancy_hierarchical_model as H
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedTrainStep, train_step
    B, N, seed, rid, nseed = 256, 16, 500, 11, 900
    rays, gt, _, _ = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, B, N, N))
    kw = {}
    if variant == "controls":
        kw = dict(background=torch.rand(B, 3, generator=torch.Generator().manual_seed(5)).to(dev), sigma_noise=0.5, noise_seed=nseed)
    net, twin = fresh(dev, synthetic), fresh(dev, synthetic)
    stepper = GraphedTrainStep(net, FusedAdam(net, lr=0.0), B, N, device_rng=True, seed=seed, ray_id0=rid, distortion=LAM_STEP,
                               storage="e4m3" if variant == "e4m3" else "bf16", **kw)
    assert stepper.distortion_weight == LAM_STEP and stepper.distortion.shape == ()
    with pytest.raises(AttributeError):
        stepper.distortion_weight = 0.1
    opt_twin = FusedAdam(twin, lr=0.0)
    seen = []
    for k in (1, 2, 3):
        loss = stepper.step(rays, gt).clone()
        dist = stepper.distortion.clone()
        ekw = dict(kw, noise_seed=nseed + k) if kw else {}
        want = train_step(twin, opt_twin, rays, gt, N, device_rng=True, seed=seed + k, ray_id0=rid, distortion=LAM_STEP, **ekw)
        assert same(loss, want) and same(dist, want.distortion), (k, float(loss), float(want), float(dist), float(want.distortion))
        assert same(stepper.mse + dist, loss) and float(dist) > 0
        seen.append(float(dist))
    assert len(set(seen)) == 3                                        # the jitter moved with the step


def test_graphed_guided_step(dev, oracle, synthetic):
    """GraphedGuidedTrainStep(distortion=) at 256 x (16 + 16), learning rate 0, three replays against the eager guided step."""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedGuidedTrainStep, train_step_guided
    B, Nc, Nf, seed, rid = 256, 16, 16, 400, 7
    rays, gt, _, _, prop = _guided_scene(dev, oracle, synthetic, B, Nc, Nf)
    net, twin = fresh(dev, synthetic), fresh(dev, synthetic)
    stepper = GraphedGuidedTrainStep(net, FusedAdam(net, lr=0.0), B, Nc, Nf, prop, device_rng=True, seed=seed, ray_id0=rid, distortion=LAM_STEP)
    assert stepper.distortion_weight == LAM_STEP
    opt_twin = FusedAdam(twin, lr=0.0)
    for k in (1, 2, 3):
        loss = stepper.step(rays, gt).clone()
        dist = stepper.distortion.clone()
        want = train_step_guided(twin, opt_twin, rays, gt, Nc, Nf, prop, device_rng=True, seed=seed + k, ray_id0=rid, distortion=LAM_STEP)
        assert same(stepper.ts_f, want.ts), k
        assert same(loss, want) and same(dist, want.distortion), (k, float(loss), float(want), float(dist), float(want.distortion))
        assert float(dist) > 0
