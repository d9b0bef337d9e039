"""Grid-guided fine sampling on the GPU (include/nerf_amd.h, "grid-guided fine sampling").  Every
comparison is exact:

  1. the look-up: sigma_c of the kernel against tests/guided_model.py, bit for bit;
  2. the kernel against the composition it is defined as, all on the GPU: nerf_amd_query_points -> model look-up (exact) ->
     nerf_amd_volume_render_rays -> nerf_amd_sample_pdf, in every sort bucket, scan carry and jitter mode;
  3. the hot path (no optional output) against the call with both, and nothing written outside the outputs;
  4. render_guided / render_guided_view against the existing render on the same positions;
  5. train_step_guided against the existing eager step on the same positions, and GraphedGuidedTrainStep against it."""
import ctypes

import numpy as np
import pytest
import torch

import guided_model as G

pytestmark = pytest.mark.gpu

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
VOLUMES = ((2, 2, 2), (5, 4, 3), (33, 17, 9))           # non-cubic: an index-order error shows
# the sort's keys-per-lane buckets (Nf <= 64, 128, 256, 512) and the scan's chunk carries (Nc - 2 across 64, 128, 192)
SIZES = ((3, 1), (64, 128), (66, 65), (67, 64), (130, 129), (194, 257), (256, 256))
MODES = ("u", "ts", "rng", "rng+seed_in_memory")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def bits(t_):
    return t_.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def make_volume(R, seed):
    """8 N(0, 1) with a solid -inf block, scattered -inf points and scattered NaN corners."""
    rng = np.random.default_rng(seed)
    V = (8 * rng.standard_normal(R)).astype(np.float32)
    V[rng.random(R) < 0.15] = -np.inf
    V[: R[0] // 3 + 1, : R[1] // 2 + 1] = -np.inf
    V[rng.random(R) < 0.1] = np.nan
    V[0, 0, 0] = V[-1, -1, 0] = np.nan
    return V


def make_rays(B, seed):
    """Unit-direction rays from radius 4 through the box (t in [2, 6] crosses it); ray 1 misses the box, ray 2 starts and
    stays inside it (a short direction), ray 3 has a zero direction component, ray 4 a NaN origin."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(B, 3, generator=g)
    o = 4 * o / o.norm(dim=1, keepdim=True)
    aim = 2 * torch.rand(B, 3, generator=g) - 1
    d = aim - o
    rays = torch.cat([o, d / d.norm(dim=1, keepdim=True)], 1)
    if B > 1:
        rays[1] = torch.tensor([4.0, 4.0, 4.0, 0.6, 0.0, 0.8])
    if B > 2:
        rays[2] = torch.tensor([0.1, 0.2, -0.3, 0.1, -0.12, 0.08])
    if B > 3:
        rays[3] = torch.tensor([0.2, 0.3, 4.0, 0.0, 0.0, -1.0])
    if B > 4:
        rays[4] = torch.tensor([float("nan"), 0.0, 4.0, 0.0, 0.0, -1.0])
    return rays.contiguous()


class Lib:
    """The entry points of the composition, on device tensors."""

    def __init__(self, dev):
        from nerf_simple_amd import _lib
        self._lib, self.lib, self.ptr, self.dev = _lib, _lib.lib(), _lib.ptr, dev
        self.f32 = dict(dtype=torch.float32, device=dev)

    def st(self):
        return self._lib.stream_ptr(self.dev)

    def query_points(self, rays, jit, tbins, flags, seed, rid, B, N):
        q, ts = torch.empty(B * N, 6, **self.f32), torch.empty(B, N, **self.f32)
        self._lib.check(self.lib.nerf_amd_query_points(self.ptr(rays), jit, self.ptr(tbins), flags, seed, rid, self.ptr(q),
                                                       self.ptr(ts), B, N, self.st()), "query_points")
        return q, ts

    def weights(self, sigma, ts, rays):
        B, N = ts.shape
        raw = torch.zeros(B, N, 4, **self.f32)
        raw[..., 3] = sigma
        outs = [torch.empty(s_, **self.f32) for s_ in ((B, 3), (B,), (B, N), (B,), (B, N))]
        self._lib.check(self.lib.nerf_amd_volume_render_rays(self.ptr(raw), self.ptr(ts), self.ptr(rays),
                                                             *[self.ptr(x) for x in outs], B, N, self.st()), "volume_render_rays")
        return outs[4]

    def sample_pdf(self, ts, w, u_f, flags, seed, rid, Nf):
        B, Nc = ts.shape
        out = torch.empty(B, Nc + Nf, **self.f32)
        self._lib.check(self.lib.nerf_amd_sample_pdf(self.ptr(ts), self.ptr(w), self.ptr(u_f), flags, seed, rid, self.ptr(out),
                                                     B, Nc, Nf, self.st()), "sample_pdf")
        return out

    def guided(self, rays, jit, tbins, flags, seed, rid, vol, lo, inv, u_f, ts_out, sigma_c, w_c, B, Nc, Nf):
        h = [(ctypes.c_float * 3)(*[float(x) for x in a]) for a in (lo, inv)]
        as_ptr = lambda x: x if not torch.is_tensor(x) else self.ptr(x)
        self._lib.check(self.lib.nerf_amd_sample_pdf_volume(
            self.ptr(rays), jit, self.ptr(tbins), flags, seed, rid, self.ptr(vol), *vol.shape, h[0], h[1], self.ptr(u_f),
            as_ptr(ts_out), as_ptr(sigma_c), as_ptr(w_c), B, Nc, Nf, self.st()), "sample_pdf_volume")


def jitter_args(L, mode, B, Nc, Nf, seed):
    """(kernel jitter pointer, tbins, kernel flags, kernel seed, u_f | None, keep-alive) and the same for the composition's
    own calls: (query jitter, query flags, query seed, sampler flags, sampler seed)."""
    _lib, dev = L._lib, L.dev
    g = torch.Generator().manual_seed(seed)
    tbins = torch.linspace(2, 6, Nc + 1).to(dev)
    u_c = torch.rand(B, Nc, generator=g).to(dev)
    u_f = torch.rand(B, max(Nf, 1), generator=g)[:, :Nf].contiguous().to(dev)
    RNG, MEM, GIVEN = _lib.FLAG_DEVICE_RNG, _lib.FLAG_SEED_IN_MEMORY, _lib.FLAG_TS_GIVEN
    s0, k = 987654321, 5
    if mode == "u":
        return dict(jit=L.ptr(u_c), tbins=tbins, flags=0, seed=0, u_f=u_f, keep=u_c,
                    q=(L.ptr(u_c), tbins, 0, 0), pdf=(0, 0))
    if mode == "ts":
        ts = ((tbins[1] - tbins[0]) * u_c + tbins[:-1]).contiguous()
        return dict(jit=L.ptr(ts), tbins=None, flags=GIVEN, seed=0, u_f=u_f, keep=ts,
                    q=(L.ptr(ts), None, GIVEN, 0), pdf=(0, 0))
    if mode == "rng":
        return dict(jit=None, tbins=tbins, flags=RNG, seed=s0, u_f=None, keep=None,
                    q=(None, tbins, RNG, s0), pdf=(RNG, s0))
    off = torch.tensor([k], dtype=torch.int64, device=dev)
    return dict(jit=L.ptr(off), tbins=tbins, flags=RNG | MEM, seed=s0, u_f=None, keep=off,
                q=(None, tbins, RNG, s0 + k), pdf=(RNG, s0 + k))


# ---- 1. the look-up --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", VOLUMES, ids=lambda r: "x".join(map(str, r)))
def test_lookup_equals_the_model(dev, R):
    L = Lib(dev)
    B, Nc, Nf, rid = 37, 66, 5, 3
    V = make_volume(R, sum(R))
    lo, _, inv = G.grid_axes(R, BOUNDS)
    rays = make_rays(B, 5).to(dev)
    a = jitter_args(L, "u", B, Nc, Nf, 17)
    qj, qtb, qflags, qseed = a["q"]
    q, ts_c = L.query_points(rays, qj, qtb, qflags, qseed, rid, B, Nc)
    vol = torch.from_numpy(V).to(dev)
    ts_out, sigma_c, w_c = (torch.full(s_, 7.0, **L.f32) for s_ in ((B, Nc + Nf), (B, Nc), (B, Nc)))
    L.guided(rays, a["jit"], a["tbins"], a["flags"], a["seed"], rid, vol, lo, inv, a["u_f"], ts_out, sigma_c, w_c, B, Nc, Nf)
    torch.cuda.synchronize(dev)
    pts = q[:, :3].cpu().numpy().reshape(B, Nc, 3)
    assert np.array_equal(pts, G.points(rays.cpu().numpy(), ts_c.cpu().numpy()), equal_nan=True)      # the model's points too
    want = G.lookup(pts, V, lo, inv)
    got = sigma_c.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # the inputs are what the test is about: inside and outside samples, NaN and -inf values met, no NaN out
    inside, _ = G.cells(pts, R, lo, inv)
    assert inside.any() and (~inside).any() and inside[2].all() and not inside[1].any() and not inside[4].any()
    assert not np.isnan(got).any() and np.isfinite(got).any()
    if R != VOLUMES[0]:                                                  # (one cell: every inside sample sees the same 8 corners)
        assert np.isneginf(got[inside]).any() and len(np.unique(got[inside])) > 4
    assert not torch.isnan(w_c).any() and not torch.isnan(ts_out).any()


# ---- 2. the kernel against the composition ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_volume(dev):
    R = VOLUMES[2]
    V = make_volume(R, 99)
    lo, _, inv = G.grid_axes(R, BOUNDS)
    return V, torch.from_numpy(V).to(dev), lo, inv


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_kernel_equals_the_composition(dev, big_volume, Nc, Nf, mode):
    L = Lib(dev)
    V, vol, lo, inv = big_volume
    rid = 17
    for B in (1, 5, 37):
        rays = make_rays(B, 100 + B).to(dev)
        a = jitter_args(L, mode, B, Nc, Nf, 1000 * Nc + Nf + B)
        qj, qtb, qflags, qseed = a["q"]
        q, ts_c = L.query_points(rays, qj, qtb, qflags, qseed, rid, B, Nc)
        sigma = torch.from_numpy(G.lookup(q[:, :3].cpu().numpy().reshape(B, Nc, 3), V, lo, inv)).to(dev)
        w_ref = L.weights(sigma, ts_c, rays)
        ts_ref = L.sample_pdf(ts_c, w_ref, a["u_f"], a["pdf"][0], a["pdf"][1], rid, Nf)
        ts_out, sigma_c, w_c = (torch.full(s_, float("nan"), **L.f32) for s_ in ((B, Nc + Nf), (B, Nc), (B, Nc)))
        L.guided(rays, a["jit"], a["tbins"], a["flags"], a["seed"], rid, vol, lo, inv, a["u_f"], ts_out, sigma_c, w_c, B, Nc, Nf)
        torch.cuda.synchronize(dev)
        tag = (B, Nc, Nf, mode)
        assert same(sigma_c, sigma), tag
        assert same(w_c, w_ref), tag
        assert same(ts_out, ts_ref), tag
        assert bool(torch.all(ts_out[:, 1:] >= ts_out[:, :-1])), tag
        if B > 1:
            assert bool(torch.all(w_c[1] == 0)), tag                    # the ray that misses the box: the uniform placement
            zeros = L.sample_pdf(ts_c, torch.zeros_like(w_ref), a["u_f"], a["pdf"][0], a["pdf"][1], rid, Nf)
            assert same(ts_out[1], zeros[1]), tag


# ---- 3. the hot path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc,Nf", ((64, 128), (67, 64)))
def test_hot_path_writes_the_same_positions_and_nothing_else(dev, big_volume, Nc, Nf):
    L = Lib(dev)
    V, vol, lo, inv = big_volume
    B, PAD, S = 37, 64, -12345.0
    rays = make_rays(B, 31).to(dev)
    a = jitter_args(L, "rng", B, Nc, Nf, 3)
    bufs = [torch.full((PAD + n + PAD,), S, **L.f32) for n in (B * (Nc + Nf), B * Nc, B * Nc, B * (Nc + Nf))]
    inner = [ctypes.c_void_p(b.data_ptr() + 4 * PAD) for b in bufs]
    args = (rays, a["jit"], a["tbins"], a["flags"], a["seed"], 9, vol, lo, inv, a["u_f"])
    L.guided(*args, inner[0], inner[1], inner[2], B, Nc, Nf)
    L.guided(*args, inner[3], None, None, B, Nc, Nf)
    L.guided(*args, inner[3], None, None, B, Nc, Nf)                    # and again: the same bytes
    torch.cuda.synchronize(dev)
    for b in bufs:
        assert bool(torch.all(b[:PAD] == S)) and bool(torch.all(b[-PAD:] == S))
        assert not bool(torch.any(b[PAD:-PAD] == S))
    assert same(bufs[0][PAD:-PAD], bufs[3][PAD:-PAD])


# ---- 4. the render ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev, oracle, synthetic):
    """A structured network, its proposal volume at 33^3 and 37 camera rays."""
    import occupancy_hierarchical_model as H
    from nerf_simple_amd.utils.nets import Nerf
    from nerf_simple_amd.utils.proposal import ProposalVolume
    net = Nerf(precision="bf16").to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, "structured"))
    prop = ProposalVolume(33, BOUNDS, device=dev)
    assert bool(torch.all(torch.isneginf(prop.sigma)))
    ptr0 = prop.sigma.data_ptr()
    prop.update(net)
    assert prop.sigma.data_ptr() == ptr0 and prop.updates == 1 and not bool(torch.isneginf(prop.sigma).any())
    rays, gt, u_c, u_f = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, 37, 16, 24))
    return dict(net=net, prop=prop, rays=rays, gt=gt, u_c=u_c, u_f=u_f, Nc=16, Nf=24)


def test_update_is_the_density_grid(dev, scene):
    from nerf_simple_amd.utils.mesh import density_grid
    from nerf_simple_amd.utils.proposal import ProposalVolume
    want = density_grid(scene["net"], 33, BOUNDS)
    assert same(scene["prop"].sigma, want)
    again = ProposalVolume.from_sigma(want, BOUNDS)
    assert again.sigma.data_ptr() == want.data_ptr() and again.resolution == (33, 33, 33)
    a = scene["prop"].sample(scene["rays"], 16, 24, u_c=scene["u_c"], u_f=scene["u_f"])
    b, sig, w = again.sample(scene["rays"], 16, 24, u_c=scene["u_c"], u_f=scene["u_f"], return_weights=True)
    assert same(a, b) and sig.shape == w.shape == (37, 16) and bool((w > 0).any())


@pytest.mark.parametrize("precision", ("fp16", "fp32"))
def test_update_in_another_precision_stays_in_place(dev, scene, precision):
    from nerf_simple_amd.utils.mesh import density_grid
    from nerf_simple_amd.utils.proposal import ProposalVolume
    prop = ProposalVolume((9, 7, 5), BOUNDS, device=dev)
    ptr0 = prop.sigma.data_ptr()
    assert prop.update(scene["net"], precision=precision) is prop and prop.sigma.data_ptr() == ptr0
    assert same(prop.sigma, density_grid(scene["net"], (9, 7, 5), BOUNDS, precision=precision))


@pytest.mark.parametrize("precision", ("fp16", "bf16", "fp32"))
def test_render_guided_is_the_render_on_its_positions(dev, scene, precision):
    from nerf_simple_amd.utils.rendering import render_guided, render_nerf
    s = scene
    with torch.no_grad():
        out = render_guided(s["rays"], s["net"], s["Nc"], s["Nf"], s["prop"], u_c=s["u_c"], u_f=s["u_f"], precision=precision)
        assert len(out) == 6
        ts = out[5]
        assert same(ts, s["prop"].sample(s["rays"], s["Nc"], s["Nf"], u_c=s["u_c"], u_f=s["u_f"]))
        want = render_nerf(s["rays"], s["net"], s["Nc"] + s["Nf"], ts=ts, precision=precision)
    for name, a, b in zip(("rgb", "disp", "alpha", "acc", "w"), out, want):
        assert same(a, b), (precision, name)


def test_render_guided_view_and_the_default_jitter(dev, scene, synthetic):
    from nerf_simple_amd.utils.rendering import generate_rays, render_guided, render_guided_view, render_nerf
    s = scene
    pose = np.eye(4, dtype=np.float32)
    pose[2, 3] = 4.0
    cam = (6, 7, 9.0)
    Nc, Nf = s["Nc"], s["Nf"]
    with torch.no_grad():
        got = render_guided_view(s["net"], pose, cam, Nc, Nf, s["prop"], device_rng=True, seed=21, precision="fp16")
        rays = generate_rays(pose, cam, dev)
        ts = s["prop"].sample(rays, Nc, Nf, device_rng=True, seed=21, ray_id0=0)
        rgb, disp, _, _, _ = render_nerf(rays, s["net"], Nc + Nf, ts=ts, precision="fp16")
        assert same(got, torch.cat([rgb.clamp(0., 1.), disp[:, None]], dim=1))
        part = render_guided_view(s["net"], pose, cam, Nc, Nf, s["prop"], device_rng=True, seed=21, precision="fp16", ray0=11,
                                  n_rays=20)
        assert same(part, got[11:31])                                    # keyed by global pixel id
        saved = torch.get_rng_state()
        try:
            B = s["rays"].shape[0]
            torch.manual_seed(78)
            st = torch.get_rng_state()
            u_c, u_f = torch.rand(B, Nc), torch.rand(B, Nf)
            want_next = torch.rand(3)
            torch.set_rng_state(st)
            out = render_guided(s["rays"], s["net"], Nc, Nf, s["prop"])
            assert torch.equal(torch.rand(3), want_next)                # advanced exactly like rand(B, Nc); rand(B, Nf)
            assert same(out[5], s["prop"].sample(s["rays"], Nc, Nf, u_c=u_c.to(dev), u_f=u_f.to(dev)))
        finally:
            torch.set_rng_state(saved)


# ---- 5. training -----------------------------------------------------------------------------------------------------------
def _net(dev, synthetic):
    from nerf_simple_amd.utils.nets import Nerf
    net = Nerf(precision="bf16").to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, "default"))
    return net


def test_train_step_guided_is_the_eager_step_on_its_positions(dev, scene, synthetic):
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import mse_loss, train_step_guided
    from nerf_simple_amd.utils.rendering import render_nerf
    s = scene
    Nc, Nf = s["Nc"], s["Nf"]
    a, b = _net(dev, synthetic), _net(dev, synthetic)
    loss = train_step_guided(a, FusedAdam(a, lr=0.0), s["rays"], s["gt"], Nc, Nf, s["prop"], u_c=s["u_c"], u_f=s["u_f"])
    ts = loss.ts
    assert not ts.requires_grad and same(ts, s["prop"].sample(s["rays"], Nc, Nf, u_c=s["u_c"], u_f=s["u_f"]))
    opt_b = FusedAdam(b, lr=0.0)
    opt_b.zero_grad(set_to_none=True)
    want = mse_loss(render_nerf(s["rays"], b, Nc + Nf, ts=ts)[0], s["gt"])
    want.backward()
    assert same(loss, want.detach())
    # the gradient reaches the network and no tensor of the proposal
    assert all(p.grad is not None for p in a.parameters()) and any(bool((p.grad != 0).any()) for p in a.parameters())
    assert not s["prop"].sigma.requires_grad and s["prop"].sigma.grad is None
    assert all(not torch.is_tensor(v) or (not v.requires_grad and v.grad is None) for v in vars(s["prop"]).values())


def test_graphed_guided_step(dev, synthetic, oracle):
    """256 rays x (16 + 16), device_rng=True, three replays against the eager guided step with seed + k.  The learning rate
    is 0: the dW products combine their split-K partial sums with float atomics, so the parameters after a non-zero
    update are not reproducible to the bit even between two runs of one stepper, and bit-equal losses over several steps
    are defined for frozen weights only.  What moves from step to step here is the seed in device memory."""
    import occupancy_hierarchical_model as H
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedGuidedTrainStep, train_step_guided
    from nerf_simple_amd.utils.proposal import ProposalVolume
    B, Nc, Nf, seed, rid = 256, 16, 16, 400, 7
    rays, gt, _, _ = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, B, Nc, Nf))
    net, twin = _net(dev, synthetic), _net(dev, synthetic)
    prop = ProposalVolume(17, BOUNDS, device=dev)
    stepper = GraphedGuidedTrainStep(net, FusedAdam(net, lr=0.0), B, Nc, Nf, prop, device_rng=True, seed=seed, ray_id0=rid)
    opt_twin = FusedAdam(twin, lr=0.0)
    unknown = ProposalVolume(17, BOUNDS, device=dev)                    # stays all -inf
    for k in (1, 2, 3):
        if k == 3:
            prop.update(net)                                            # in place, between two replays
        loss = stepper.step(rays, gt).clone()
        ts_f = stepper.ts_f.clone()
        want = train_step_guided(twin, opt_twin, rays, gt, Nc, Nf, prop, device_rng=True, seed=seed + k, ray_id0=rid)
        assert same(loss, want), k
        assert same(ts_f, want.ts), k
        blind = unknown.sample(rays, Nc, Nf, device_rng=True, seed=seed + k, ray_id0=rid)
        assert same(ts_f, blind) == (k < 3), k                          # the update changed the positions of the next step
    # the sigma tensor's address is baked into the graph
    prop.sigma = prop.sigma.clone()
    with pytest.raises(RuntimeError, match="replaced"):
        stepper.step(rays, gt)
