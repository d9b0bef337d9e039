"""The per-image colour correction on the GPU: the four stages against the torch expressions that define them
(tests/appearance_model.py), the reduction against float64 with its derived bound, the affine head against the five-stage
composition bit for bit and against float64 by the model's constants, the eager chain through render_nerf against float64
oracle autograd (tests/input_grad_model.py's rules), GraphedAppearanceTrainStep step by step against the hand-made chain of
the same entry points, and the recovery of known corrections over three images against the factors the fp32 CPU loop reaches."""
import numpy as np
import pytest
import torch

import appearance_model as AM
import input_grad_model as IG
import ray_routines_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _call(name, *args):
    """One C entry point on the current stream; tensors and None become pointers."""
    from nerf_simple_amd import _lib
    a = [_lib.ptr(x) if torch.is_tensor(x) or x is None else x for x in args]
    _lib.check(getattr(_lib.lib(), name)(*a, _lib.stream_ptr(torch.device(DEV, 0))), name)


def _same(got, want):
    """torch.equal with NaN meeting NaN (the bad rays)."""
    got, want = got.cpu(), want.cpu()
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))


def _f32(**kw):
    return dict(dtype=torch.float32, device=DEV, **kw)


# ---- the stages ------------------------------------------------------------------------------------------------------------------
S_B, S_M, S_HW = 37, 4, 16


def _stage_inputs():
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(0, S_HW, (S_B,), generator=g) + S_HW * torch.tensor([0, 1, 3])[torch.randint(0, 3, (S_B,), generator=g)]
    ids[4], ids[20] = -1, S_M * S_HW                         # the two bad ids; image 2 has no ray; repeats are certain at 37 of 48
    ids[9] = ids[8]
    theta = torch.cat([torch.rand(S_M, 3, generator=g) * 0.6 - 0.3, torch.rand(S_M, 3, generator=g) * 0.1 - 0.05], dim=1)
    return ids, theta, torch.randn(S_B, 3, generator=g), torch.randn(S_B, 3, generator=g)


def test_stages_are_the_torch_expressions():
    ids, theta, rgb, g_out = _stage_inputs()
    bad = ~AM.valid_rows(ids, S_M, S_HW)
    assert int(bad.sum()) == 2 and 2 not in set((ids[~bad] // S_HW).tolist()) and len(set(ids.tolist())) < S_B
    rows = torch.full((S_B, 6), 7.0, device=DEV)
    kept = torch.full((S_B,), -5, dtype=torch.int64, device=DEV)
    _call("nerf_amd_appearance_gather", theta.to(DEV), ids.to(DEV), kept, S_HW, rows, S_B, S_M)
    want_rows = AM.gather(theta, ids, S_HW)
    assert torch.equal(kept.cpu(), ids) and _same(rows, want_rows)
    assert bool(torch.isnan(rows.cpu()[bad]).all()) and not bool(torch.isnan(rows.cpu()[~bad]).any())
    rows2 = torch.full((S_B, 6), 7.0, device=DEV)
    _call("nerf_amd_appearance_gather", theta.to(DEV), ids.to(DEV), None, S_HW, rows2, S_B, S_M)      # no copy asked for
    assert _same(rows2, want_rows)
    one = theta[1].contiguous()
    for stride, r_dev, r_cpu in ((6, rows, want_rows), (0, one.to(DEV), one)):
        out = torch.full((S_B, 3), 7.0, device=DEV)
        _call("nerf_amd_appearance_apply", rgb.to(DEV), r_dev, stride, out, S_B)
        want = AM.apply(rgb, r_cpu)
        assert _same(out, want), stride
        nan_rays = torch.isnan(out.cpu()).any(dim=1)
        assert torch.equal(nan_rays, bad if stride == 6 else torch.zeros_like(bad)), stride         # NaN only in the bad rays
        g_rgb, g_ray = torch.full((S_B, 3), 7.0, device=DEV), torch.full((S_B, 6), 7.0, device=DEV)
        _call("nerf_amd_appearance_apply_backward", g_out.to(DEV), rgb.to(DEV), r_dev, stride, g_rgb, g_ray, S_B)
        want_rgb, want_ray = AM.apply_backward(g_out, rgb, r_cpu)
        assert _same(g_rgb, want_rgb) and _same(g_ray, want_ray), stride
        assert not bool(torch.isnan(g_ray).any())             # (g rgb, g) does not look at theta
        # in place: out over rgb, g_rgb over g_out
        c, gg = rgb.to(DEV).clone(), g_out.to(DEV).clone()
        _call("nerf_amd_appearance_apply_backward", gg, c, r_dev, stride, gg, g_ray, S_B)
        _call("nerf_amd_appearance_apply", c, r_dev, stride, c, S_B)
        assert _same(c, want) and _same(gg, want_rgb), stride


# ---- the reduction ---------------------------------------------------------------------------------------------------------------
R_B = 1000


def _reduce(g_ray, ids, theta, reg, frozen):
    out = torch.full((theta.shape[0], 6), 7.0, device=DEV)    # written, not accumulated
    mask = None
    if frozen:
        mask = torch.zeros(theta.shape[0], dtype=torch.int32, device=DEV)
        mask[list(frozen)] = 1
    _call("nerf_amd_appearance_reduce", g_ray.to(DEV), ids.to(DEV), S_HW, theta.to(DEV), float(reg), mask, out, ids.shape[0],
          theta.shape[0])
    return out.cpu()


@pytest.mark.parametrize("reg,frozen", [(0.0, ()), (0.25, (1,))])
def test_reduction(reg, frozen):
    """1000 rows (four passes of the block's 256 threads) over images 0, 1 and 3 of 4, two bad ids: within the derived bound of
    the float64 sum (appearance_model.reduce64), two runs equal bytes, one call = a call per image within the same bound, frozen
    rows exactly 0, the absent image exactly reg * theta."""
    g = torch.Generator().manual_seed(23)
    ids = torch.randint(0, S_HW, (R_B,), generator=g) + S_HW * torch.tensor([0, 1, 3])[torch.randint(0, 3, (R_B,), generator=g)]
    ids[5], ids[700] = S_M * S_HW + 3, -7
    g_ray, theta = torch.randn(R_B, 6, generator=g), torch.randn(S_M, 6, generator=g)
    g_ray[5], g_ray[700] = float("nan"), 1e30                  # what a bad ray carries reaches no image
    want, bound = AM.reduce64(g_ray, ids, S_HW, theta, reg, frozen)
    got = _reduce(g_ray, ids, theta, reg, frozen)
    err = np.abs(got.double().numpy() - want)
    print(f"reduction reg={reg}: worst |err| / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g} over "
          f"{int(AM.valid_rows(ids, S_M, S_HW).sum())} rows")
    assert (err <= bound).all(), (err, bound)
    assert torch.equal(got.view(torch.int32), _reduce(g_ray, ids, theta, reg, frozen).view(torch.int32))
    for m in frozen:
        assert torch.equal(got[m].view(torch.int32), torch.zeros(6, dtype=torch.int32))         # +0, no ridge
    assert torch.equal(got[2], torch.tensor(reg) * theta[2])                                     # absent: reg * theta exactly
    for m in range(S_M):                                       # the rows of one image alone, in their own thread assignment
        pick = torch.div(ids, S_HW, rounding_mode="floor") == m
        alone = _reduce(g_ray[pick], ids[pick], theta, reg, frozen) if bool(pick.any()) else None
        if alone is not None:
            assert (np.abs(alone[m].double().numpy() - want[m]) <= bound[m]).all(), m


# ---- the head --------------------------------------------------------------------------------------------------------------------
def _head(raw, ts, rays, target, rows, stride=6):
    B, N = ts.shape
    rgb, g_ray, d_raw = (torch.full(s, float("nan"), device=DEV) for s in ((B, 3), (B, 6), (B, N, 4)))      # an unwritten row shows
    _call("nerf_amd_volume_render_mse_backward_affine", raw, ts, rays, target, rows, stride, rgb, g_ray, d_raw, B, N)
    return rgb, g_ray, d_raw


def _composition(raw, ts, rays, target, rows, stride=6):
    """compositor (rgb) -> apply -> g' = 2 (c' - target) / (3 B) -> apply_backward -> compositor backward (g_rgb only)."""
    B, N = ts.shape
    rgb, disp, acc = torch.empty((B, 3), **_f32()), torch.empty((B,), **_f32()), torch.empty((B,), **_f32())
    _call("nerf_amd_volume_render_rays", raw, ts, rays, rgb, disp, None, acc, None, B, N)
    pred = torch.empty_like(rgb)
    _call("nerf_amd_appearance_apply", rgb, rows, stride, pred, B)
    g = AM.mse_gradient(pred, target).contiguous()
    g_rgb, g_ray, d_raw = torch.empty_like(rgb), torch.empty((B, 6), **_f32()), torch.full((B, N, 4), float("nan"), device=DEV)
    _call("nerf_amd_appearance_apply_backward", g, rgb, rows, stride, g_rgb, g_ray, B)
    _call("nerf_amd_volume_render_rays_backward", raw, ts, rays, g_rgb, None, None, None, None, d_raw, B, N)
    return pred, g_ray, d_raw


@pytest.fixture(scope="module")
def head_inputs():
    """appearance_model.head_inputs of every case (and of N = 1), on the device, with the rows gathered by the kernel."""
    out = {}
    for kind in AM.HEAD_KINDS:
        for N in (1,) + AM.HEAD_N:
            raw, ts, rays, target, theta, ids = AM.head_inputs(kind, N)
            rows = torch.empty((AM.HEAD_B, 6), **_f32())
            _call("nerf_amd_appearance_gather", theta.to(DEV), ids.to(DEV), None, AM.HEAD_HW, rows, AM.HEAD_B, AM.HEAD_M)
            out[(kind, N)] = tuple(x.to(DEV).contiguous() for x in (raw, ts, rays, target)) + (rows,)
    return out


@pytest.mark.parametrize("kind", AM.HEAD_KINDS)
@pytest.mark.parametrize("N", (1,) + AM.HEAD_N)
def test_head_is_the_composition(head_inputs, kind, N):
    """rgb, g_theta_ray and d_raw of the ONE launch equal the five-stage composition, at a row per ray and at one row for all; a
    NaN sigma in one ray and a NaN row (a bad id) in another leave every other ray's bytes unchanged; theta = 0 gives the plain
    head's d_raw; N = 1 is the closed form of the empty sample axis."""
    raw, ts, rays, target, rows = head_inputs[(kind, N)]
    B = AM.HEAD_B
    for stride, r in ((6, rows), (0, rows[3].clone())):
        got, want = _head(raw, ts, rays, target, r, stride), _composition(raw, ts, rays, target, r, stride)
        for name, a, b in zip(("rgb", "g_theta_ray", "d_raw"), got, want):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (name, stride)
    rgb, g_ray, d_raw = _head(raw, ts, rays, target, rows)
    if N == 1:
        zero = torch.zeros(B, 3, device=DEV)
        pred = AM.apply(zero, rows)
        g = AM.mse_gradient(pred, target)
        assert torch.equal(rgb, pred) and not bool(d_raw.any()) and torch.equal(g_ray, torch.cat([g * zero, g], dim=1))
    # a NaN sigma in ray 5, a NaN row in ray 7: loud there, every other ray bit for bit what it is alone
    raw2, rows2 = raw.clone(), rows.clone()
    raw2[5, N // 2, 3] = float("nan")
    rows2[7] = float("nan")
    rgb2, g_ray2, d_raw2 = _head(raw2, ts, rays, target, rows2)
    others = torch.ones(B, dtype=torch.bool, device=DEV)
    others[[5, 7]] = False
    for a, b in ((rgb, rgb2), (g_ray, g_ray2), (d_raw, d_raw2)):
        assert torch.equal(a[others].view(torch.int32), b[others].view(torch.int32))
    assert bool(torch.isnan(rgb2[7]).all()) and bool(torch.isnan(g_ray2[7]).all())
    if N > 1:               # (the empty sample axis has no sample to receive anything: d_raw = 0 there by definition)
        assert bool(torch.isnan(d_raw2[7]).all()) and bool(torch.isnan(d_raw2[5]).any())
    # theta = 0: fl(1 + 0) c + 0 = c -- the plain head's d_raw (and rgb), with either stride
    rgb_p, d_p = torch.empty_like(rgb), torch.full_like(d_raw, float("nan"))
    _call("nerf_amd_volume_render_mse_backward", raw, ts, rays, target, rgb_p, d_p, B, N)
    for stride, r in ((6, torch.zeros_like(rows)), (0, torch.zeros(6, device=DEV))):
        rgb0, _, d0 = _head(raw, ts, rays, target, r, stride)
        assert torch.equal(d0, d_p) and torch.equal(rgb0, rgb_p), stride


@pytest.mark.parametrize("kind", AM.HEAD_KINDS)
def test_head_against_float64(head_inputs, kind):
    """d_raw by the compositor backward's per-ray rule (ray_ratios, bound = 2 c + 4) with the constants appearance_model.py
    measures on the reference's own fp32 error on these cases.  c' within 64 EPS max(1, |c'|) of float64 (the rule
    tests/test_gpu_background.py gives rgb_bg).  The ray's row of g_theta = (g' c, g') with g' = 2 (c' - t) / (3 B): c and c'
    each carry those 64 EPS R (R = max(1, |c|, |c'|)), the difference, the two factors and the product one rounding each, so
    |err g'| <= (2 / 3B)(64 + 4) EPS R and |err g' c| <= R |err g'| + |g'| 64 EPS R + EPS |g' c| <= (2 / 3B) 200 EPS R^2 with
    |c' - t| <= 2 R."""
    worst, failed = {}, []
    for N in AM.HEAD_N:
        raw, ts, rays, target, rows = head_inputs[(kind, N)]
        rgb, g_ray, d_raw = _head(raw, ts, rays, target, rows)
        cpu = [x.cpu() for x in (raw, ts, rays, target, rows)]
        want, A, pred64, g_ray64, rgb64 = AM.head_model(*cpu)
        keep = np.isfinite(AM.oracle_head_grad(*cpu, torch.float32)[0])
        got = d_raw.cpu().numpy()
        assert np.isfinite(got[keep]).all(), N
        R = max(1.0, float(np.abs(pred64).max()), float(np.abs(rgb64).max()))
        assert np.abs(rgb.cpu().double().numpy() - pred64).max() <= 64 * AM.EPS * R, N
        assert np.abs(g_ray.cpu().double().numpy() - g_ray64).max() <= (2 / (3 * AM.HEAD_B)) * 200 * AM.EPS * R * R, N
        cond, plain = M.ray_ratios(got, want, A, keep)
        for key, r, limit in (("conditioned", float(cond.max()), M.bound(AM.C_REF_APP)),
                              ("plain", float(np.nanmax(plain, initial=0.0)), M.bound(AM.C_REF_APP_PLAIN))):
            if key not in worst or r / limit > worst[key][0] / worst[key][1]:
                worst[key] = (r, limit, N)
            if not r <= limit:
                failed.append((N, key, r, limit))
    print(f"affine head vs float64, {kind}: " + ", ".join(f"{k} {v[0]:.2f} of {v[1]:.1f} (N={v[2]})" for k, v in worst.items()))
    assert not failed, failed


# ---- the eager chain -------------------------------------------------------------------------------------------------------------
E_TENSOR = "color_fc.2.weight"


def _net(sd, precision, frozen=True):
    from nerf_simple_amd.utils.nets import Nerf
    net = Nerf(precision=precision).to(DEV)
    net.load_state_dict(sd)
    net.requires_grad_(not frozen)
    return net


@pytest.fixture(scope="module")
def chain_truth():
    """3 images of 8 x 8, N = 16: d MSE((1 + a) rgb + b, target) / d theta and / d one network tensor by oracle autograd in
    float64, fp32 and the bf16 emulation (with the parameter gradients' own roundings: train_heads)."""
    import nerf_oracle as O
    from nerf_simple_amd.utils import synthetic
    sd = synthetic.synthetic_state_dict(0, "structured")
    cam, N = [8, 8, synthetic.focal_from_fov(8)], 16
    table = torch.cat([O.camera_rays(torch.from_numpy(O.spherical_to_pose(*p)).float(), cam) for p in AM.REC_POSES])
    g = torch.Generator().manual_seed(21)
    ids = torch.randperm(3 * 64, generator=g)
    u = torch.rand(len(ids), N, generator=g)
    target = torch.rand(len(ids), 3, generator=g)
    theta0 = torch.cat([torch.rand(3, 3, generator=g) * 0.6 - 0.3, torch.rand(3, 3, generator=g) * 0.1 - 0.05], dim=1)
    rays = table[ids].contiguous()
    grads = {}
    for name, fwd, dt in (("g64", IG.exact_forward, torch.float64), ("g32", IG.exact_forward, torch.float32),
                          ("g16", lambda s, v: IG.emulated_forward(s, v, train_heads=True), torch.float32)):
        sdd = {k: t.to(dt).clone().requires_grad_(k == E_TENSOR) for k, t in sd.items()}
        theta = theta0.to(dt).clone().requires_grad_(True)
        rgb = IG.render(fwd, sdd, rays.to(dt), N, u=u)[0]
        torch.nn.functional.mse_loss(AM.apply(rgb, AM.gather(theta, ids, 64)), target.to(dt)).backward()
        grads[name] = (theta.grad.detach(), sdd[E_TENSOR].grad.detach())
    return dict(sd=sd, N=N, rays=rays, ids=ids, u=u, target=target, theta0=theta0, **grads)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_eager_chain_gradient(chain_truth, precision):
    from nerf_simple_amd import training
    from nerf_simple_amd.utils.appearance import AppearanceCorrection
    from nerf_simple_amd.utils.rendering import render_nerf
    t = chain_truth
    net = _net(t["sd"], precision, frozen=False)
    app = AppearanceCorrection(3, 64, DEV)
    with torch.no_grad():
        app.theta.copy_(t["theta0"])
    rgb = render_nerf(t["rays"].to(DEV), net, t["N"], u=t["u"].to(DEV), precision=precision)[0]
    loss = training.mse_loss(app(rgb, t["ids"].to(DEV)), t["target"].to(DEV))
    loss.backward()
    got = (app.theta.grad, dict(net.named_parameters())[E_TENSOR].grad)
    for k, name in enumerate(("theta", E_TENSOR)):
        g64, g32, g16 = t["g64"][k], t["g32"][k], t["g16"][k]
        bound = IG.bound_fp32(g32, g64) if precision == "fp32" else IG.bound_bf16(g16, g32, g64)
        err = IG.rel_err(got[k], g64)
        print(f"eager chain {precision}: {name} grad rel err {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (name, err, bound)
    # the module's own surface
    assert torch.equal(app.gains(), 1 + app.theta.detach()[:, :3]) and torch.equal(app.bias(), app.theta.detach()[:, 3:])
    other = AppearanceCorrection(3, 64, DEV)
    other.load_state_dict(app.state_dict())
    assert torch.equal(other.theta, app.theta) and list(app.state_dict()) == ["theta"]
    with pytest.raises(RuntimeError, match="one colour per ray id"):
        app(rgb[:5], t["ids"].to(DEV))
    with pytest.raises(RuntimeError, match="int64"):
        app(rgb, t["ids"].to(DEV).int())


# ---- the graphed step ------------------------------------------------------------------------------------------------------------
G_B, G_N, G_M, G_SIDE, G_LR, G_SEED = 256, 16, 4, 8, 2e-3, 40


def _generator(poses, cam, colours):
    from nerf_simple_amd.utils.dataload import RayGenerator
    H, W = cam[0], cam[1]
    imgs = colours.reshape(len(poses), H, W, 3).cpu().numpy()
    return RayGenerator.from_samples({"train": [{"img": im, "transform": p.numpy()} for im, p in zip(imgs, poses)]}, cam, DEV)


def _graphed_setup(device_rng=True, storage="bf16", **kw):
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedAppearanceTrainStep
    from nerf_simple_amd.utils import synthetic
    from nerf_simple_amd.utils.appearance import AppearanceCorrection
    from nerf_simple_amd.utils.xyz import spherical_to_pose
    cam = [G_SIDE, G_SIDE, synthetic.focal_from_fov(G_SIDE)]
    poses = torch.stack([torch.from_numpy(spherical_to_pose(4, -30 - 5 * m, 90 * m)).float() for m in range(G_M)])
    colours = torch.rand(G_M * G_SIDE * G_SIDE, 3, generator=torch.Generator().manual_seed(5))
    rg = _generator(poses, cam, colours)
    net = _net(synthetic.synthetic_state_dict(0, "default"), "bf16", frozen=False)
    app = AppearanceCorrection.from_ray_generator(rg, reg=0.125, frozen=(2,))
    assert (app.M, app.HW) == (G_M, G_SIDE * G_SIDE)
    stepper = GraphedAppearanceTrainStep(net, FusedAdam(net, lr=0.0), G_B, G_N, app, rays_from=rg, appearance_lr=G_LR,
                                         device_rng=device_rng, seed=G_SEED, storage=storage, **kw)
    return stepper, rg


def _hand_chain(stepper, rg, theta, ids, k):
    """The step's entry points by hand on ``ids`` with the corrections ``theta``: gather -> the training forward (jitter of
    step k, the stepper's storage form) -> affine head -> loss value -> reduce.  Returns (loss, g_theta)."""
    from nerf_simple_amd import _lib
    lib, B, N = _lib.lib(), stepper.B, stepper.N
    P, app = B * N, stepper.appearance
    f32, u8 = _f32(), dict(dtype=torch.uint8, device=DEV)
    rays, gt = rg.rays_dataset["train"][ids].contiguous(), rg.colours["train"][ids].contiguous()
    rows = torch.empty((B, 6), **f32)
    _call("nerf_amd_appearance_gather", theta, ids, None, app.HW, rows, B, app.M)
    raw, ts, d_raw, rgb = torch.empty((B, N, 4), **f32), torch.empty((B, N), **f32), torch.empty((B, N, 4), **f32), torch.empty((B, 3), **f32)
    e4m3 = stepper.storage == "e4m3"
    acts = torch.empty(int((lib.nerf_amd_train_activation_bytes_e4m3 if e4m3 else lib.nerf_amd_train_activation_bytes)(P)), **u8)
    store = _lib.FLAG_STORE_E4M3 if e4m3 else 0
    if stepper.device_rng:
        jit, flags, seed = None, _lib.FLAG_DEVICE_RNG, stepper.seed + k
    else:
        jit, flags, seed = stepper.u, 0, 0
    _call("nerf_amd_mlp_forward_train", rays, jit, stepper.tbins, stepper._packed_fwd, flags | store, seed, 0, raw, ts, acts, B, N)
    g_ray, loss, g_theta = torch.empty((B, 6), **f32), torch.zeros((), **f32), torch.empty_like(theta)
    _call("nerf_amd_volume_render_mse_backward_affine", raw, ts, rays, gt, rows, 6, rgb, g_ray, d_raw, B, N)
    _call("nerf_amd_mse_loss", rgb, gt, loss, None, B * 3)
    _call("nerf_amd_appearance_reduce", g_ray, ids, app.HW, theta, app.reg, app._frozen_arg, g_theta, B, app.M)
    return loss, g_theta


@pytest.mark.parametrize("device_rng,storage", [(True, "bf16"), (False, "bf16"), (True, "e4m3")])
def test_graphed_step_is_the_hand_made_chain(device_rng, storage):
    """Three replays at 256 rays x 16 samples, 4 images of 8 x 8 (one frozen, a ridge of 0.125), network rate 0: the loss,
    appearance_grad, theta and the ids of every step equal the chain of the same entry points -- the second Adam by hand as
    well, nerf_amd_adam_step_hyper on moments carried here with the scalars the stepper documents -- bit for bit."""
    from nerf_simple_amd.training import GraphedTrainStep
    stepper, rg = _graphed_setup(device_rng, storage)
    app = stepper.appearance
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        app.theta.copy_(torch.cat([torch.rand(G_M, 3, generator=g) * 0.4 - 0.2, torch.rand(G_M, 3, generator=g) * 0.1 - 0.05], dim=1))
    hand = app.theta.detach().clone()
    m, v = torch.zeros_like(hand), torch.zeros_like(hand)
    b1, b2 = stepper.appearance_betas
    torch.manual_seed(3)
    for k in (1, 2, 3):
        before = app.theta.detach().clone()
        assert torch.equal(before, hand), k
        loss = stepper.step().clone()
        torch.cuda.synchronize()
        ids = stepper.ray_ids.clone()
        assert sorted(ids.tolist()) == list(range(G_B))                                          # B = n: a permutation
        assert torch.equal(ids, GraphedTrainStep.ray_ids.fget(stepper)), k                       # the selection's own record
        want_loss, want_grad = _hand_chain(stepper, rg, before, ids, k)
        assert torch.equal(loss, want_loss) and bool(torch.isfinite(loss)), (k, float(loss), float(want_loss))
        assert torch.equal(stepper.appearance_grad, want_grad), k
        assert bool(stepper.appearance_grad[[0, 1, 3]].any()) and not bool(stepper.appearance_grad[2].any())
        hyper = torch.tensor([G_LR, b1, b2, 1e-8, 1.0 - b1 ** k, (1.0 - b2 ** k) ** 0.5, 0.0, 0.0], dtype=torch.float32, device=DEV)
        _call("nerf_amd_adam_step_hyper", hand, want_grad, m, v, hand.numel(), hyper)
        assert torch.equal(app.theta.detach(), hand) and not torch.equal(hand, before), k
        assert torch.equal(app.theta.detach()[2], before[2])                                     # the frozen image does not move
    assert stepper.appearance_steps == 3


def test_graphed_step_refusals_and_schedule():
    from nerf_simple_amd.training import GraphedAppearanceTrainStep
    from nerf_simple_amd.utils.appearance import AppearanceCorrection
    from nerf_simple_amd.utils.dataload import RayGenerator
    stepper, rg = _graphed_setup()
    net, opt, app = stepper.net, stepper.opt, stepper.appearance
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="takes no rays"):
        stepper.step(torch.zeros(G_B, 6, device=DEV), torch.zeros(G_B, 3, device=DEV))
    for kw, match in ((dict(background=torch.zeros(3)), "background"), (dict(sigma_noise=0.1), "sigma_noise"),
                      (dict(distortion=0.01), "distortion")):
        with pytest.raises(RuntimeError, match=match):
            GraphedAppearanceTrainStep(net, opt, G_B, G_N, app, rays_from=rg, **kw)
    with pytest.raises(RuntimeError, match="required"):
        GraphedAppearanceTrainStep(net, opt, G_B, G_N, app, rays_from=None)
    with pytest.raises(RuntimeError, match="span"):
        GraphedAppearanceTrainStep(net, opt, G_B, G_N, AppearanceCorrection(3, G_SIDE * G_SIDE, DEV), rays_from=rg)
    bare = RayGenerator.from_tables(rg.rays_dataset["train"])
    with pytest.raises(RuntimeError, match="colour"):
        GraphedAppearanceTrainStep(net, opt, G_B, G_N, app, rays_from=bare)
    assert torch.equal(torch.get_rng_state(), state)
    stepper.step(appearance_decay=0.5, decay=1.0)
    assert stepper.appearance_lr == G_LR * 0.5
    app.theta.data = app.theta.data.clone()                     # the tensor the graph writes is no longer the module's
    with pytest.raises(RuntimeError, match="replaced"):
        stepper.step()


# ---- recovery --------------------------------------------------------------------------------------------------------------------
def _recovery_scene(precision):
    """(frozen net, rays of every pixel, ids, the fixed jitter, target colours through theta*, cam, poses)."""
    from nerf_simple_amd.utils.rendering import generate_rays, render_nerf
    sd, poses, cam = AM.recovery_scene()
    net = _net(sd, precision)
    rays = torch.cat([generate_rays(p, cam, DEV) for p in poses])
    ids = torch.arange(3 * AM.REC_HW, device=DEV)
    u = AM.recovery_jitter().to(DEV)
    with torch.no_grad():
        target = AM.recovery_target(render_nerf(rays, net, AM.REC_N, u=u)[0])
    return net, rays, ids, u, target, cam, poses


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_recovery_eager(precision):
    """Three images of 12 x 12, image 0 frozen at the identity, true gains in [0.7, 1.3] and biases within +-0.05; targets =
    the frozen net's own render through theta*; one torch Adam (lr 0.02) on app.theta from zero for 40 steps, fixed jitter.
    The fp32 CPU loop cuts ||theta - theta*|| by appearance_model.RECOVERY_F_FIXED; the GPU must reach half of it."""
    from nerf_simple_amd import training
    from nerf_simple_amd.utils.appearance import AppearanceCorrection
    from nerf_simple_amd.utils.rendering import render_nerf
    net, rays, ids, u, target, _, _ = _recovery_scene(precision)
    app = AppearanceCorrection(3, AM.REC_HW, DEV, frozen=AM.REC_FROZEN)
    opt = torch.optim.Adam([app.theta], AM.REC_LR)
    e0 = AM.recovery_error(app.theta)
    for _ in range(AM.REC_STEPS):
        opt.zero_grad()
        training.mse_loss(app(render_nerf(rays, net, AM.REC_N, u=u)[0], ids), target).backward()
        opt.step()
    e1 = AM.recovery_error(app.theta)
    print(f"eager recovery {precision}: ||theta - theta*|| {e0:.4g} -> {e1:.4g}, factor {e0 / e1:.3g} "
          f"(the fp32 CPU loop: {AM.RECOVERY_F_FIXED})")
    assert not bool(app.theta.detach()[0].any())
    assert e1 * AM.RECOVERY_F_FIXED / 2 <= e0, (e0, e1)


def test_recovery_graphed():
    """The same scene inside the captured step: B = n = 432 rays, fresh counter-RNG jitter per step, network rate 0, 40 replays.
    The fp32 CPU loop with a fresh torch.rand draw per step cuts ||theta - theta*|| by appearance_model.RECOVERY_F_FRESH; the
    GPU (bf16 operands, other jitter) must reach half of it."""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedAppearanceTrainStep
    from nerf_simple_amd.utils.appearance import AppearanceCorrection
    net, _, _, _, target, cam, poses = _recovery_scene("bf16")
    net.requires_grad_(True)
    rg = _generator(poses, cam, target)
    app = AppearanceCorrection.from_ray_generator(rg, frozen=AM.REC_FROZEN)
    stepper = GraphedAppearanceTrainStep(net, FusedAdam(net, lr=0.0), app.n_rays, AM.REC_N, app, rays_from=rg,
                                         appearance_lr=AM.REC_LR, device_rng=True, seed=1)
    e0 = AM.recovery_error(app.theta)
    for _ in range(AM.REC_STEPS):
        stepper.step()
    e1 = AM.recovery_error(app.theta)
    print(f"graphed recovery: ||theta - theta*|| {e0:.4g} -> {e1:.4g}, factor {e0 / e1:.3g} (the fp32 CPU loop: {AM.RECOVERY_F_FRESH})")
    assert not bool(app.theta.detach()[0].any())
    assert e1 * AM.RECOVERY_F_FRESH / 2 <= e0, (e0, e1)
