"""GPU tests of the hierarchical training step (BASELINE config 4 trained: MSE(rgb_c, gt) + MSE(rgb_f, gt), the fine
positions placed by sample_pdf on the DETACHED coarse weights).  The reference has no hierarchical path, so parity is
unpinned against it; the pair is pinned against the oracle's composition (oracle.render_nerf -> oracle.sample_pdf ->
oracle.render_nerf) and its pieces against the library's own single-network step.

  * the coarse head kernel (nerf_amd_volume_render_mse_backward_pdf) is bit for bit the composition
    nerf_amd_volume_render_mse_backward + nerf_amd_volume_render_rays (w) + nerf_amd_sample_pdf;
  * precision='fp32' pair: losses, fine positions and all 48 gradient tensors against float64 autograd;
  * bf16 pair: gradients inside the rel-L2 bound model of tests/test_gpu_training.py (P = B*Nc coarse, B*(Nc+Nf) fine);
  * stop-gradient: the coarse net's gradients are train_step's on the coarse pass alone;
  * GraphedHierarchicalTrainStep equals the eager step (both jitter modes) and leaves a usable pair behind."""
import numpy as np
import pytest
import torch

from test_gpu_training import rel_l2, rel_l2_bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _pair(dev, precision, seeds=(0, 1), kind="default"):
    from nerf_simple_amd.utils.nets import Nerf
    nets = []
    for s in seeds:
        n = Nerf(precision=precision).to(dev)
        n.load_state_dict(_sd(s, kind))
        nets.append(n)
    return nets


def _sd(seed, kind="default"):
    from nerf_simple_amd.utils import synthetic
    return synthetic.synthetic_state_dict(seed, kind)


def _head_inputs(B, Nc, dev, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(B, Nc, 4, generator=g) * 2.0
    raw[..., 3] = raw[..., 3] * 4.0                       # densities from empty to opaque
    u = torch.rand(B, Nc, generator=g)
    bins = torch.linspace(2.0, 6.0, Nc + 1)
    ts = (bins[1] - bins[0]) * u + bins[:-1]
    rays = torch.randn(B, 6, generator=g)
    target = torch.rand(B, 3, generator=g)
    return [x.contiguous().to(dev) for x in (raw, ts, rays, target)]


# Nc in {3, 64, 65, 256} x Nf in {0, 1, 128, 256}, plus the 8-keys-per-lane sort bucket (Nf > 256) at the limit Nc + Nf <= 512
HEAD_CASES = [(nc, nf) for nc in (3, 64, 65, 256) for nf in (0, 1, 128, 256)] + [(64, 448), (3, 509)]


@pytest.mark.parametrize("Nc,Nf", HEAD_CASES)
def test_coarse_head_equals_composition(dev, Nc, Nf):
    """rgb, d_raw and ts_out of the one-launch coarse head against the three entry points it fuses, bit for bit, with
    explicit jitter, the counter RNG (seed as argument) and the counter RNG with the seed offset in device memory."""
    from nerf_simple_amd import _lib
    assert Nc + Nf <= 512
    lib, ptr = _lib.lib(), _lib.ptr
    st = _lib.stream_ptr(dev)
    for B in ((37, 4096) if (Nc, Nf) == (64, 128) else (37,)):
        raw, ts, rays, target = _head_inputs(B, Nc, dev, 1000 * Nc + Nf + B)
        f32 = dict(dtype=torch.float32, device=dev)
        rgb_ref, d_raw_ref = torch.empty(B, 3, **f32), torch.empty(B, Nc, 4, **f32)
        _lib.check(lib.nerf_amd_volume_render_mse_backward(ptr(raw), ptr(ts), ptr(rays), ptr(target), ptr(rgb_ref),
                                                           ptr(d_raw_ref), B, Nc, st), "mse_backward")
        outs = [torch.empty(s_, **f32) for s_ in ((B, 3), (B,), (B, Nc), (B,), (B, Nc))]
        _lib.check(lib.nerf_amd_volume_render_rays(ptr(raw), ptr(ts), ptr(rays), *[ptr(x) for x in outs], B, Nc, st),
                   "volume_render_rays")
        w = outs[4]
        u_f = torch.rand(B, max(Nf, 1), generator=torch.Generator().manual_seed(Nf + B)).to(dev)[:, :Nf].contiguous()
        seed, rid0, k = 1234567, 17, 5
        off = torch.tensor([k], dtype=torch.int64, device=dev)
        # (head flags, head u, head seed) and the sample_pdf call it must equal
        modes = [(0, ptr(u_f), 0, 0, ptr(u_f), 0),
                 (_lib.FLAG_DEVICE_RNG, None, seed, _lib.FLAG_DEVICE_RNG, None, seed),
                 (_lib.FLAG_DEVICE_RNG | _lib.FLAG_SEED_IN_MEMORY, ptr(off), seed, _lib.FLAG_DEVICE_RNG, None, seed + k)]
        for hflags, hu, hseed, pflags, pu, pseed in modes:
            ts_ref = torch.empty(B, Nc + Nf, **f32)
            _lib.check(lib.nerf_amd_sample_pdf(ptr(ts), ptr(w), pu, pflags, pseed, rid0, ptr(ts_ref), B, Nc, Nf, st), "sample_pdf")
            rgb, d_raw, ts_out = torch.full((B, 3), np.nan, **f32), torch.full((B, Nc, 4), np.nan, **f32), \
                torch.full((B, Nc + Nf), np.nan, **f32)
            _lib.check(lib.nerf_amd_volume_render_mse_backward_pdf(ptr(raw), ptr(ts), ptr(rays), ptr(target), hu, hflags, hseed,
                                                                   rid0, ptr(rgb), ptr(d_raw), ptr(ts_out), B, Nc, Nf, st),
                       "volume_render_mse_backward_pdf")
            torch.cuda.synchronize(dev)
            tag = (B, Nc, Nf, hflags)
            assert torch.equal(rgb, rgb_ref), tag
            assert torch.equal(rgb, outs[0]), tag
            assert torch.equal(d_raw, d_raw_ref), tag
            assert torch.equal(ts_out, ts_ref), tag
            assert bool(torch.all(ts_out[:, 1:] >= ts_out[:, :-1])), tag


def _oracle_pair(oracle, sd_c, sd_f, rays, gt, u_c, u_f, Nc, Nf, dtype, ts_f=None):
    """Autograd through oracle.render_nerf -> oracle.sample_pdf on the detached weights -> oracle.render_nerf(ts), in
    ``dtype``.  The coarse positions are the fp32 stratified ones (oracle.sample_ts on fp32 u: torch's, bit for bit the
    GPU's), and ``ts_f`` (the GPU's fine positions) if given: the positional encoding's 2^9 frequencies turn fp32 position
    rounding into ~1e-4 gradient differences that are the inputs', not the arithmetic's.  The oracle's own fine positions
    are returned for a check of their own."""
    pc = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd_c.items()}
    pf = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd_f.items()}
    rays, gt = rays.to(dtype), gt.to(dtype)
    ts_c = oracle.sample_ts(u_c.float(), 2, 6).to(dtype)
    coarse = oracle.render_nerf(rays, pc, Nc, ts=ts_c)
    own_ts_f = oracle.sample_pdf(ts_c, coarse[4].detach(), u_f.to(dtype))
    fine = oracle.render_nerf(rays, pf, Nc + Nf, ts=(own_ts_f if ts_f is None else ts_f.to(dtype)))
    lc = torch.nn.functional.mse_loss(coarse[0], gt)
    lf = torch.nn.functional.mse_loss(fine[0], gt)
    (lc + lf).backward()
    return (float(lc.detach()), float(lf.detach())), {k: p.grad for k, p in pc.items()}, {k: p.grad for k, p in pf.items()}, \
        own_ts_f


def _pair_step(dev, nets, rays, gt, u_c, u_f, Nc, Nf):
    from nerf_simple_amd.training import train_step_hierarchical
    net_c, net_f = nets
    opt = torch.optim.SGD(list(net_c.parameters()) + list(net_f.parameters()), lr=0.0)
    loss = train_step_hierarchical(net_c, net_f, opt, rays.to(dev), gt.to(dev), Nc, Nf, u_c=u_c.to(dev), u_f=u_f.to(dev))
    gc = {k: p.grad.detach().float().cpu() for k, p in net_c.named_parameters()}
    gf = {k: p.grad.detach().float().cpu() for k, p in net_f.named_parameters()}
    return loss, gc, gf


def test_pair_fp32_exact_vs_oracle(dev, golden, oracle):
    """precision='fp32' pair (layer by layer, fp32 end to end) against float64 autograd of the oracle composition at the
    same sample positions, with tests/error_model.py's fp32 model: the oracle's own fp32 result sits e_ref from the
    float64 truth (per gradient tensor, relative L2); the GPU -- the same arithmetic in another summation order -- is
    allowed FACTOR_32 = 2 x e_ref + a floor of a few fp32 ulps times sqrt(B*N) for the dW sums' order (1e-5).  The
    fine positions against the oracle's own sample_pdf of its float64 coarse weights: fp32 round-off (1e-4 abs in [2, 6])."""
    from error_model import FACTOR_32
    g = golden("train.npz")
    B, Nc, Nf = 16, 16, 32
    rays, gt = t(g["rays"])[:B], t(g["gt"])[:B]
    gen = torch.Generator().manual_seed(5)
    u_c, u_f = torch.rand(B, Nc, generator=gen), torch.rand(B, Nf, generator=gen)
    loss, gc, gf = _pair_step(dev, _pair(dev, "fp32"), rays, gt, u_c, u_f, Nc, Nf)
    ts_gpu = loss.ts_f.cpu()
    (lc, lf), wc, wf, ts_f = _oracle_pair(oracle, _sd(0), _sd(1), rays, gt, u_c, u_f, Nc, Nf, torch.float64, ts_f=ts_gpu)
    (lc32, lf32), rc, rf, _ = _oracle_pair(oracle, _sd(0), _sd(1), rays, gt, u_c, u_f, Nc, Nf, torch.float32, ts_f=ts_gpu)
    got_l = [float(x) for x in loss.losses]
    for got, want, ref32 in zip(got_l, (lc, lf), (lc32, lf32)):
        assert abs(got - want) <= FACTOR_32 * abs(ref32 - want) + 4 * 2.0 ** -24 * abs(want), (got_l, lc, lf, lc32, lf32)
    assert float((ts_gpu.double() - ts_f).abs().max()) <= 1e-4
    worst = []
    for tag, got, want, ref32 in (("c", gc, wc, rc), ("f", gf, wf, rf)):
        for k in want:
            e_ref = rel_l2(ref32[k].double().numpy(), want[k].numpy())
            e_gpu = rel_l2(got[k].numpy(), want[k].numpy())
            worst.append((e_gpu / (FACTOR_32 * e_ref + 1e-5), f"{tag}:{k}", e_gpu, e_ref))
    worst.sort()
    print("fp32 pair: worst gradient tensor (error / bound, name, GPU rel L2, oracle fp32 rel L2):", worst[-1])
    assert len(worst) == 48
    assert worst[-1][0] <= 1.0, worst[-5:]


def test_pair_bf16_vs_oracle_fp32(dev, golden, oracle):
    """The bf16 pair against the oracle's fp32 composition fed the GPU's own fine positions: both networks' gradients
    inside the rel-L2 bound model of tests/test_gpu_training.py, P = B*Nc (coarse) and B*(Nc+Nf) (fine)."""
    g = golden("train.npz")
    B, Nc, Nf = 64, 64, 128
    rays, gt = t(g["rays"]), t(g["gt"])
    gen = torch.Generator().manual_seed(6)
    u_c, u_f = t(g["u"]), torch.rand(B, Nf, generator=gen)
    loss, gc, gf = _pair_step(dev, _pair(dev, "bf16"), rays, gt, u_c, u_f, Nc, Nf)
    (lc, lf), wc, wf, _ = _oracle_pair(oracle, _sd(0), _sd(1), rays, gt, u_c, u_f, Nc, Nf, torch.float32,
                                       ts_f=loss.ts_f.cpu())
    got_l = [float(x) for x in loss.losses]
    assert abs(got_l[0] - lc) <= 1e-3 * lc and abs(got_l[1] - lf) <= 1e-3 * lf, (got_l, lc, lf)
    for got, want, P in ((gc, wc, B * Nc), (gf, wf, B * (Nc + Nf))):
        worst = {k: rel_l2(got[k].numpy(), want[k].numpy()) for k in want}
        print(f"bf16 pair P={P}: rel L2 max {max(worst.values()):.3e} ({max(worst, key=worst.get)})")
        assert max(worst.values()) <= rel_l2_bound("default", P), worst


def test_coarse_gradients_stop_at_the_weights(dev, golden):
    """The coarse net learns from MSE(rgb_c, gt) alone: its gradients from the pair step are train_step's on the coarse
    pass (same u_c, Nc) up to the dW atomics' order, and do not move when the fine net's weights change."""
    from nerf_simple_amd.training import train_step
    g = golden("train.npz")
    B, Nc, Nf = 64, 64, 128
    rays, gt, u_c = t(g["rays"]).to(dev), t(g["gt"]).to(dev), t(g["u"]).to(dev)
    u_f = torch.rand(B, Nf, generator=torch.Generator().manual_seed(7)).to(dev)
    _, gc1, _ = _pair_step(dev, _pair(dev, "bf16", (0, 1)), rays, gt, u_c, u_f, Nc, Nf)
    _, gc2, _ = _pair_step(dev, _pair(dev, "bf16", (0, 2), kind="default"), rays, gt, u_c, u_f, Nc, Nf)
    single = _pair(dev, "bf16", (0,))[0]
    train_step(single, torch.optim.SGD(single.parameters(), lr=0.0), rays, gt, Nc, u=u_c)
    gs = {k: p.grad.detach().float().cpu() for k, p in single.named_parameters()}
    for k in gs:
        assert rel_l2(gc1[k].numpy(), gs[k].numpy()) <= 1e-5, k
        assert rel_l2(gc2[k].numpy(), gs[k].numpy()) <= 1e-5, k


def _run_pair(dev, graphed, steps, rays, gt, Nc, Nf, decay, us=None, device_rng=False, seed=0):
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import train_step_hierarchical, GraphedHierarchicalTrainStep
    net_c, net_f = _pair(dev, "bf16")
    opt = FusedAdam([net_c, net_f], lr=5e-4)
    losses = []
    if graphed:
        stepper = GraphedHierarchicalTrainStep(net_c, net_f, opt, rays.shape[0], Nc, Nf, device_rng=device_rng, seed=seed)
        for i in range(steps):
            kw = {} if us is None else dict(u_c=us[i][0], u_f=us[i][1])
            loss = stepper.step(rays, gt, decay=decay, **kw)
            losses.append((float(loss), [float(x) for x in stepper.losses]))
    else:
        stepper = None
        for i in range(steps):
            kw = dict(device_rng=True, seed=seed + i + 1) if device_rng else dict(u_c=us[i][0], u_f=us[i][1])
            loss = train_step_hierarchical(net_c, net_f, opt, rays, gt, Nc, Nf, decay=decay, **kw)
            losses.append((float(loss), [float(x) for x in loss.losses]))
    assert opt.step_count == steps
    with torch.no_grad():
        probe = torch.cat([net_c(rays[:8].new_zeros(8, 6) + 0.1), net_f(rays[:8].new_zeros(8, 6) - 0.1)]).cpu()
    return losses, opt.flat.detach().cpu().clone(), probe, (net_c, net_f, opt, stepper)


def _assert_same_run(a, b):
    (la, pa, qa, _), (lb, pb, qb, _) = a, b
    tot_a, tot_b = [x[0] for x in la], [x[0] for x in lb]
    assert tot_a[-1] < tot_a[0] and tot_b[-1] < tot_b[0]
    np.testing.assert_allclose(tot_a, tot_b, rtol=2e-3)
    np.testing.assert_allclose([x[1] for x in la], [x[1] for x in lb], rtol=2e-3)
    for (tot, (c, f)) in lb:
        assert abs(tot - (c + f)) <= 1e-6 * tot
    d = (pa - pb).abs()
    assert float(d.max()) <= 6 * 5e-4 and float(d.mean()) <= 1e-5 and float((d > 1e-5).float().mean()) <= 0.06
    assert float((qa - qb).abs().max()) <= 2e-2 * max(1.0, float(qa.abs().max()))


def test_graphed_pair_matches_eager(dev, golden):
    """6 decayed steps of GraphedHierarchicalTrainStep against train_step_hierarchical with FusedAdam([net_c, net_f]) on
    the same rays / jitter: losses, parameters and a probe forward within the tolerances of
    test_graphed_train_step_matches_eager.  Then one step without jitter: the CPU generator is drawn like torch.rand(B,Nc)
    followed by torch.rand(B,Nf)."""
    from nerf_simple_amd.training import lr_decay_factor
    g = golden("train.npz")
    B, Nc, Nf = 64, 64, 128
    rays, gt = t(g["rays"]).to(dev), t(g["gt"]).to(dev)
    decay = lr_decay_factor(5e-4, 4e-4, 10)
    gen = torch.Generator().manual_seed(11)
    us = [(torch.rand(B, Nc, generator=gen).to(dev), torch.rand(B, Nf, generator=gen).to(dev)) for _ in range(6)]
    eager = _run_pair(dev, False, 6, rays, gt, Nc, Nf, decay, us=us)
    graphed = _run_pair(dev, True, 6, rays, gt, Nc, Nf, decay, us=us)
    _assert_same_run(eager, graphed)
    net_c, net_f, opt, stepper = graphed[3]
    assert abs(opt.param_groups[0]["lr"] - 5e-4 * decay ** 6) < 1e-12
    saved = torch.get_rng_state()
    try:
        torch.manual_seed(78)
        st = torch.get_rng_state()
        want_c, want_f = torch.rand(B, Nc), torch.rand(B, Nf)
        want_next = torch.rand(3)
        torch.set_rng_state(st)
        stepper.step(rays, gt)
        assert torch.equal(stepper.u_c.cpu(), want_c) and torch.equal(stepper.u_f.cpu(), want_f)
        assert torch.equal(torch.rand(3), want_next)
    finally:
        torch.set_rng_state(saved)


def test_graphed_pair_device_rng_matches_eager(dev, golden):
    """device_rng=True: step k of the graph draws both passes' jitter with seed + k, the eager step's values with
    seed=seed + k."""
    from nerf_simple_amd.training import lr_decay_factor
    g = golden("train.npz")
    rays, gt = t(g["rays"]).to(dev), t(g["gt"]).to(dev)
    decay = lr_decay_factor(5e-4, 4e-4, 10)
    eager = _run_pair(dev, False, 6, rays, gt, 64, 128, decay, device_rng=True, seed=900)
    graphed = _run_pair(dev, True, 6, rays, gt, 64, 128, decay, device_rng=True, seed=900)
    _assert_same_run(eager, graphed)


def test_trained_pair_renders(dev, golden):
    """After graphed steps render_hierarchical_view sees the updated weights: its pixels equal those of a fresh pair
    loaded with the trained state dicts."""
    from nerf_simple_amd.utils.rendering import render_hierarchical_view
    g = golden("train.npz")
    rays, gt = t(g["rays"]).to(dev), t(g["gt"]).to(dev)
    _, _, _, (net_c, net_f, opt, stepper) = _run_pair(dev, True, 3, rays, gt, 64, 128, 1.0, device_rng=True, seed=3)
    pose = np.eye(4, dtype=np.float32)
    pose[2, 3] = 4.0
    cam = (24, 24, 30.0)
    got = render_hierarchical_view(net_c, net_f, pose, cam, 64, 128, device_rng=True, seed=9, precision="bf16")
    fresh = _pair(dev, "bf16")
    fresh[0].load_state_dict(net_c.state_dict())
    fresh[1].load_state_dict(net_f.state_dict())
    want = render_hierarchical_view(fresh[0], fresh[1], pose, cam, 64, 128, device_rng=True, seed=9, precision="bf16")
    untrained = render_hierarchical_view(*_pair(dev, "bf16"), pose, cam, 64, 128, device_rng=True, seed=9, precision="bf16")
    assert torch.equal(got, want)
    assert not torch.equal(got, untrained)


def test_pair_errors(dev):
    """The graphed step takes FusedAdam([net_c, net_f]) of the same pair, bf16 modules only."""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedHierarchicalTrainStep, train_step_hierarchical
    net_c, net_f = _pair(dev, "bf16")
    other = _pair(dev, "bf16", (2,))[0]
    with pytest.raises(ValueError):
        FusedAdam([net_c, net_c])
    with pytest.raises(RuntimeError, match="optimizer"):
        GraphedHierarchicalTrainStep(net_c, net_f, FusedAdam([net_c, other]), 8, 64, 128)
    with pytest.raises(RuntimeError, match="optimizer"):
        GraphedHierarchicalTrainStep(net_c, net_f, FusedAdam(net_c), 8, 64, 128)
    with pytest.raises(RuntimeError, match="optimizer"):
        train_step_hierarchical(net_c, net_f, FusedAdam([net_f, net_c]), torch.zeros(8, 6, device=dev),
                                torch.zeros(8, 3, device=dev))
    c32, f32 = _pair(dev, "fp32")
    with pytest.raises(RuntimeError, match="bf16"):
        GraphedHierarchicalTrainStep(c32, f32, FusedAdam([c32, f32]), 8, 64, 128)
    state = torch.get_rng_state()
    for Nc, Nf in ((2, 16), (64, 449)):
        with pytest.raises(ValueError):
            train_step_hierarchical(net_c, net_f, FusedAdam([c32, f32]), torch.zeros(8, 6, device=dev),
                                    torch.zeros(8, 3, device=dev), Nc, Nf)
    assert torch.equal(torch.get_rng_state(), state)


def test_fused_adam_pair_is_one_flat_vector(dev):
    """FusedAdam([net_c, net_f]): one flat vector, coarse first; the lr loop of the reference works; one step moves both
    modules and re-packs both images."""
    from nerf_simple_amd import _lib
    from nerf_simple_amd.optim import FusedAdam
    net_c, net_f = _pair(dev, "bf16")
    opt = FusedAdam([net_c, net_f], lr=1e-3)
    n = int(_lib.lib().nerf_amd_param_count())
    assert opt.flat.numel() == 2 * n == 1191688
    assert next(net_c.parameters()).data_ptr() == opt.flat.data_ptr()
    assert next(net_f.parameters()).data_ptr() == opt.flat.data_ptr() + 4 * n
    for pg in opt.param_groups:
        pg["lr"] *= 0.5
    before = [m.packed_weights(_lib.BF16).clone() for m in (net_c, net_f)]
    for p in list(net_c.parameters()) + list(net_f.parameters()):
        p.grad = torch.ones_like(p)
    opt.step()
    after = [m.packed_weights(_lib.BF16) for m in (net_c, net_f)]
    assert all(not torch.equal(a, b) for a, b in zip(before, after))
    for m, sl in zip((net_c, net_f), opt.slices):
        fresh = _pair(dev, "bf16", (3,))[0]
        fresh.load_state_dict(m.state_dict())
        assert torch.equal(fresh.packed_weights(_lib.BF16), m.packed_weights(_lib.BF16))


def test_graphed_pair_selects_its_own_rays(dev, oracle, synthetic, golden):
    """GraphedHierarchicalTrainStep(rays_from=RayGenerator.from_tables(...)) in both jitter modes: the rows it trains on are
    those GraphedTrainStep selects for the same seed / generator state, and each step equals the pair fed that batch by
    hand.  (a) device_rng=True: the selection is a node of graph A, one step ahead; (b) the reference stream: the ids are
    torch.randperm's, then torch.rand(B,Nc), torch.rand(B,Nf) from the same stream, the generator left where they leave it."""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedTrainStep, GraphedHierarchicalTrainStep
    from nerf_simple_amd.utils.dataload import RayGenerator
    d = golden("dataset.npz")
    hw = int(d["hw"])
    rays_tab = torch.cat([oracle.camera_rays(torch.from_numpy(oracle.spherical_to_pose(4, -30, float(phi))).float(),
                                             [hw, hw, synthetic.focal_from_fov(hw)]) for phi in d["views"]]).contiguous()
    gt_tab = torch.from_numpy(np.ascontiguousarray(d["gt"]))
    n, B, Nc, Nf = rays_tab.shape[0], 256, 64, 128
    rg = RayGenerator.from_tables(rays_tab, gt_tab, device=dev)

    def pair(**kw):
        net_c, net_f = _pair(dev, "bf16")
        return GraphedHierarchicalTrainStep(net_c, net_f, FusedAdam([net_c, net_f], lr=5e-4), B, Nc, Nf, **kw)

    def single(**kw):
        net = _pair(dev, "bf16", (0,))[0]
        return GraphedTrainStep(net, FusedAdam(net, lr=5e-4), B, Nc, **kw)

    # (a) counter RNG, selection inside the graph
    auto, hand, one = pair(device_rng=True, seed=11, rays_from=rg), pair(device_rng=True, seed=11), \
        single(device_rng=True, seed=11, rays_from=rg)
    for step in (1, 2, 3):
        la = float(auto.step())
        one.step()
        want = torch.from_numpy(oracle.select_ids_counter(n, B, 11, step))
        assert torch.equal(auto.ray_ids.cpu(), want), step
        assert torch.equal(one.ray_ids.cpu(), want), step
        lb = float(hand.step(rays_tab[want].to(dev), gt_tab[want].to(dev)))
        assert la == lb if step == 1 else abs(la - lb) <= 1e-4 * abs(lb), (step, la, lb)
    assert float((auto.opt.flat - hand.opt.flat).abs().max()) <= 3 * 5e-4
    with pytest.raises(RuntimeError):
        auto.step(rays_tab[:B].to(dev), gt_tab[:B].to(dev))
    # (b) the reference's stream
    saved = torch.get_rng_state()
    try:
        ref, byhand, one = pair(rays_from=rg), pair(), single(rays_from=rg)
        torch.manual_seed(5)
        for step in range(3):
            st = torch.get_rng_state()
            ids, u_c, u_f = torch.randperm(n)[:B], torch.rand(B, Nc), torch.rand(B, Nf)
            after = torch.get_rng_state()
            torch.set_rng_state(st)
            one.step()                                   # GraphedTrainStep from the same generator state
            torch.set_rng_state(st)
            lc = float(ref.step())
            assert torch.equal(ref.ray_ids.cpu(), ids), step
            assert torch.equal(one.ray_ids.cpu(), ids), step
            assert torch.equal(ref.u_c.cpu(), u_c) and torch.equal(ref.u_f.cpu(), u_f), step
            assert torch.equal(torch.get_rng_state(), after), step
            ld = float(byhand.step(rays_tab[ids].to(dev), gt_tab[ids].to(dev), u_c=u_c.to(dev), u_f=u_f.to(dev)))
            assert lc == ld if step == 0 else abs(lc - ld) <= 1e-4 * abs(ld), (step, lc, ld)
        assert float((ref.opt.flat - byhand.opt.flat).abs().max()) <= 3 * 5e-4
    finally:
        torch.set_rng_state(saved)
