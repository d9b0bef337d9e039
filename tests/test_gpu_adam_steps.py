"""Adam and the graphed steppers' per-step scalars, step by step (model: tests/adam_model.py).

B1  the three Adam kernels against the float64 element model, every element of p, m, v inside a bound derived from the
    kernel's operation count, at sizes on both sides of a wave, a workgroup and the 4096 x 256 grid the kernels stride by;
B2  forty steps of every kind of graphed stepper: after each, the scalars in ``stepper.hyper`` are the model's bit for bit,
    the update is nerf_amd_adam_step_hyper on the stepper's own stored gradient with a hyper vector the TEST built, bit for
    bit, and the packed training images are a fresh pack of the new weights, byte for byte;
B3  the device jitter's key across the ring's wrap;
B4  a host exception between the replay and the ring's bookkeeping does not make the next step train on another slot.

Nothing here has a tolerance of its own: B1's bounds are the model's, everything else is an equality of bits or bytes."""
import numpy as np
import pytest
import torch

import adam_model as A
import grad_guard_model as G
import occupancy_hierarchical_model as H
import occupancy_model as OM

pytestmark = pytest.mark.gpu

BETAS, EPS, LR = (0.9, 0.999), 1e-8, 5e-4
GRID = 4096 * 256                                   # the threads of an Adam launch: elements behind it are a second trip
N_PAIR = 2 * 595844
SENTINEL, GUARD_WORDS = 0x7fc0dead, 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---- B1: the kernels against the model ------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 255, 256, 257, GRID - 1, GRID, GRID + 1, N_PAIR, 2 * GRID + 3)
STEPS = ((1, LR), (2, LR), (1000, LR), (1000, 0.0))            # (t, lr): three consecutive steps, then one with lr = 0
CORNERS = (0.0, 1e-23, 1e19, 1e21)
# g = 0 on v = 0 (0 / (0 + eps): no update); |g| = 1e-23 ((1 - b2) g^2 = 1e-49 is below the smallest subnormal: v stays 0);
# g = 1e19 (the issue's: its square, 1e38, and (1 - b2) g^2 = 1e35 are still finite in fp32 -- pinned by the bound like any
# element); g = 1e21 ((1 - b2) g^2 = 1e39 overflows: the model states v = +inf and an update of exactly 0).
VARIANTS = ("plain", "hyper", "guarded coef 1", "guarded coef 0.5")


def corner_places(n):
    """Element 0, element n - 1 and both sides of index GRID, four elements each (one per corner), where they exist."""
    want = list(range(0, 4)) + list(range(n - 4, n)) + list(range(GRID - 4, GRID + 4))
    return sorted({i for i in want if 0 <= i < n})


class Buffers:
    """p, m, v and g of one kernel variant on the device, each followed by GUARD_WORDS sentinel words."""

    def __init__(self, p, n, dev):
        self.n = n
        self.full = [torch.full((n + GUARD_WORDS,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32) for _ in range(4)]
        self.p, self.m, self.v, self.g = (f[:n] for f in self.full)
        self.p.copy_(p)
        self.m.zero_()
        self.v.zero_()

    def sentinels_survive(self):
        return all(bool((f[self.n:].view(torch.int32) == SENTINEL).all()) for f in self.full)


@pytest.mark.parametrize("n", SIZES)
def test_kernels_against_the_model(dev, n):
    """nerf_amd_adam_step, nerf_amd_adam_step_hyper and nerf_amd_adam_step_guarded (coef 1; coef 0.5 on the gradient doubled,
    an exact product, so one model serves all four) on the same inputs: |got - model| / bound <= 1 for every element of p, m,
    v; +inf and an untouched parameter exactly where the model says fp32 overflows; lr = 0 leaves every parameter's bits; the
    plain and the hyper kernel write the same bits when the latter is fed adam_model.scalars of the former's arguments; the
    sentinels behind every buffer survive.  The worst ratio per output is printed: an output, not a tolerance."""
    from nerf_simple_amd import _lib
    gen = torch.Generator().manual_seed(1000 + n % 9973)
    p0 = torch.randn(n, generator=gen) * torch.pow(10.0, torch.rand(n, generator=gen) * 6 - 6)
    state = {name: Buffers(p0, n, dev) for name in VARIANTS}
    hyper = torch.zeros(8, dtype=torch.float32, device=dev)
    records = {}
    for name, coef in (("guarded coef 1", 1.0), ("guarded coef 0.5", 0.5)):
        records[name] = torch.zeros(8, dtype=torch.float32, device=dev)
        records[name][2] = coef                                       # word 3 (skip) stays 0
    places = corner_places(n)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for k, (t, lr) in enumerate(STEPS):
        g = torch.randn(n, generator=gen) * torch.pow(10.0, torch.rand(n, generator=gen) * 8 - 8)
        for rank, i in enumerate(places):
            g[i] = CORNERS[(rank + k) % 4] * (-1.0 if (rank // 4) % 2 else 1.0)
        s = A.scalars(lr, BETAS, EPS, t)
        hyper[:6] = torch.from_numpy(s)
        idx = torch.tensor(places, device=dev)
        for name, b in state.items():
            if lr != 0.0:                                             # each corner starts from empty moments (g = 0 on v = 0) ...
                b.m[idx] = 0.0                                        # ... but the lr = 0 step inherits them, an inf v included
                b.v[idx] = 0.0
            b.g.copy_(g * 2.0 if name == "guarded coef 0.5" else g)
        models, rated = [], []                    # one model per distinct input state, one rating per distinct output
        for name, b in state.items():
            before = [x.clone() for x in (b.p, b.m, b.v)]
            if name == "plain":
                _lib.launch("nerf_amd_adam_step", b.p, b.g, b.m, b.v, n, lr, BETAS[0], BETAS[1], EPS, t, dev=dev)
            elif name == "hyper":
                _lib.launch("nerf_amd_adam_step_hyper", b.p, b.g, b.m, b.v, n, hyper, dev=dev)
            else:
                _lib.launch("nerf_amd_adam_step_guarded", b.p, b.g, b.m, b.v, n, hyper, records[name], dev=dev)
            res = next((r for held, r in models if all(same_bits(x, y) for x, y in zip(held, before))), None)
            if res is None:
                res = A.step(*(x.cpu().numpy() for x in before), g.numpy(), s)
                models.append((before, res))
                assert not res.ambiguous.any()
                inf_at = [i for rank, i in enumerate(places) if CORNERS[(rank + k) % 4] == 1e21]
                if lr != 0.0:
                    assert list(np.flatnonzero(res.v_inf)) == inf_at, (t, inf_at)
                else:
                    assert set(inf_at) <= set(np.flatnonzero(res.v_inf).tolist())
            after = (b.p, b.m, b.v)
            r = next((r for m_, out, r in rated if m_ is res and all(same_bits(x, y) for x, y in zip(out, after))), None)
            got = [x.cpu().numpy() for x in after]
            if r is None:
                r = A.ratios(res, *got)
                rated.append((res, [x.clone() for x in after], r))
            print(f"n={n} t={t} lr={lr} {name}: worst |got - model| / bound  p {r['p']:.3f}  m {r['m']:.3f}  v {r['v']:.3f}")
            assert max(r.values()) <= 1.0, (name, t, r)
            assert np.all(np.isposinf(got[2][res.v_inf])) and np.array_equal(got[0][res.v_inf], before[0].cpu().numpy()[res.v_inf])
            if lr == 0.0:
                assert same_bits(b.p, before[0]), name
            assert b.sentinels_survive(), name
            worst = {key: max(worst[key], r[key]) for key in worst}
        for x, y in zip((state["plain"].p, state["plain"].m, state["plain"].v), (state["hyper"].p, state["hyper"].m, state["hyper"].v)):
            assert same_bits(x, y), ("plain vs hyper", t)
    print(f"n={n}: worst ratios over all steps and kernels  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")


# ---- B2: forty graphed steps, each rebuilt from its stored gradient ---------------------------------------------------------------
B2_STEPS = 40


def make_net(dev, synthetic, seed=0):
    from nerf_simple_amd.utils.nets import Nerf
    net = Nerf(precision="bf16").to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(seed, "default"))
    return net


def own_hyper(words, dev):
    """The 8 words the test computed, as the device vector an Adam launch reads."""
    return torch.from_numpy(words.copy()).view(torch.float32).to(dev)


def check_adam(what, hyper, counter, lr, betas, eps, t, word67, before, grad, state, dev):
    """The three checks on one Adam of a stepper: the scalars the replay ran with, the ring's counter, the update."""
    from nerf_simple_amd import _lib
    want = A.hyper_words(A.scalars(lr, betas, eps, t), word67)
    got = hyper.view(torch.int32).cpu().numpy()
    assert np.array_equal(got, want), (what, t, got.view(np.float32)[:6], want.view(np.float32)[:6], got[6:], want[6:],
                                        [j for j in range(8) if got[j] != want[j]])
    assert int(counter.item()) == t, (what, t, int(counter.item()))
    _lib.launch("nerf_amd_adam_step_hyper", before[0], grad, before[1], before[2], before[0].numel(), own_hyper(want, dev), dev=dev)
    for got_t, ref, name in zip(state, before, ("params", "exp_avg", "exp_avg_sq")):
        assert same_bits(got_t, ref), (what, t, name)


def check_images(stepper, t):
    """Both packed training images are a fresh pack of ``opt.flat`` into new buffers, byte for byte; the forward image's
    256-byte status block is excepted (the backward image has none)."""
    from nerf_simple_amd import _lib
    lib = _lib.lib()
    for net, flat, bufs in stepper._images:
        fresh = [torch.full_like(b, 0xA5) for b in bufs]
        _lib.launch("nerf_amd_pack_weights", flat, fresh[0], _lib.BF16, dev=stepper.dev)      # an image is initialised once ...
        _lib.launch("nerf_amd_pack_weights_train", flat, fresh[0], fresh[1], dev=stepper.dev)  # ... and re-packed as a step does
        for got, want, code in zip(bufs, fresh, (_lib.BF16, _lib.BF16_BWD)):
            off = int(lib.nerf_amd_packed_status_offset(code))
            assert got.numel() == want.numel() == int(lib.nerf_amd_packed_bytes(code))
            if off < 0:
                assert torch.equal(got, want), (t, "backward image")
            else:
                assert off + 256 == got.numel() and torch.equal(got[:off], want[:off]), (t, "forward image")


class Checked:
    """A stepper and how to step it, with the B2 checks behind every step."""

    def __init__(self, stepper, run, table_kw=None):
        self.stepper, self.run, self.table_kw = stepper, run, table_kw
        self.opt = stepper.opt
        self.pg = self.opt.param_groups[0]
        self.state = (self.opt.flat, self.opt.exp_avg, self.opt.exp_avg_sq)
        self.a2 = getattr(stepper, "_adam2", None)

    def snapshot(self):
        self.before = [x.clone() for x in self.state]
        self.lr = self.pg["lr"]
        if self.a2 is not None:
            self.before2 = [x.detach().clone() for x in (self.a2.table, self.a2.m, self.a2.v)]
            self.lr2 = self.a2.lr

    def check(self):
        s, opt, a2 = self.stepper, self.opt, self.a2
        torch.cuda.synchronize()
        t = opt.step_count
        grad = s.grads
        if opt.guard is not None:                                      # the rebuilt step uses the record's coef
            rec = opt.guard.cpu().numpy()
            coef = G.coef(rec[0], rec[1])
            assert rec[2].tobytes() == np.float32(coef).tobytes() and rec.view(np.int32)[3] == 0, (t, rec)
            grad = grad if coef == 1 else grad * float(coef)
            self.coef = float(coef)
        check_adam("network", s.hyper, s._ring.counter, self.lr, self.pg["betas"], self.pg["eps"], t, t, self.before, grad,
                   self.state, s.dev)
        if a2 is not None:
            check_adam("table", a2.hyper, a2.ring.counter, self.lr2, a2.betas, a2.eps, a2.steps, 0, self.before2, a2.grad,
                       (a2.table, a2.m, a2.v), s.dev)
        check_images(s, t)

    def step(self, decay):
        self.snapshot()
        loss = self.run(self.stepper, decay)
        self.check()
        return loss


def dense_scene(dev, oracle, synthetic, B=64, N=8):
    rays, gt, u, _ = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, B, N, 4))
    return rays, gt, u


def image_table(dev, oracle, synthetic):
    """The table of tests/test_gpu_graphed_launch_order.py: 3 images of 5 x 5 pixels, 75 rows for a batch of 37."""
    from nerf_simple_amd.utils.dataload import RayGenerator
    M, side = 3, 5
    cam = [side, side, synthetic.focal_from_fov(side)]
    colours = torch.rand(M, side, side, 3, generator=torch.Generator().manual_seed(5)).numpy()
    poses = [np.asarray(oracle.spherical_to_pose(4, -30 - 5 * m, 90 * m), dtype=np.float32) for m in range(M)]
    return RayGenerator.from_samples({"train": [{"img": im, "transform": p} for im, p in zip(colours, poses)]}, cam, dev)


KINDS = ("plain", "device_rng", "guarded", "pair", "masked", "camera", "appearance")
TABLE_LR = {"camera": "camera_lr", "appearance": "appearance_lr"}


def build(kind, dev, oracle, synthetic, check_every=3):
    """A Checked stepper of ``kind`` at the grad-guard tests' size (64 rays x 8 samples; 32 x (8 + 8) for the pair; the table
    steppers at their own tests' 37 rays from 75 rows), lr = 5e-4."""
    from nerf_simple_amd import training as T
    from nerf_simple_amd.optim import FusedAdam
    kw = dict(check_every=check_every)
    if kind == "pair":
        B, Nc, Nf = 32, 8, 8
        rays, gt, u_c, u_f = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, B, Nc, Nf))
        nets = [make_net(dev, synthetic, s) for s in (0, 1)]
        stepper = T.GraphedHierarchicalTrainStep(nets[0], nets[1], FusedAdam(nets, lr=LR), B, Nc, Nf, **kw)
        assert stepper.grads.numel() == N_PAIR > GRID                 # the grid-stride tail, inside a graph
        return Checked(stepper, lambda s, decay: s.step(rays, gt, u_c=u_c, u_f=u_f, decay=decay))
    net = make_net(dev, synthetic)
    if kind in TABLE_LR:
        from nerf_simple_amd.utils.appearance import AppearanceCorrection
        from nerf_simple_amd.utils.cameras import CameraRefinement
        rg = image_table(dev, oracle, synthetic)
        opt = FusedAdam(net, lr=LR)
        if kind == "camera":
            stepper = T.GraphedCameraTrainStep(net, opt, 37, 8, CameraRefinement.from_ray_generator(rg), rays_from=rg,
                                               device_rng=True, seed=11, camera_lr=2e-3, **kw)
            return Checked(stepper, lambda s, decay: s.step(decay=decay, camera_decay=decay))
        stepper = T.GraphedAppearanceTrainStep(net, opt, 37, 8, AppearanceCorrection.from_ray_generator(rg), rays_from=rg,
                                               device_rng=True, seed=11, appearance_lr=2e-3, **kw)
        return Checked(stepper, lambda s, decay: s.step(decay=decay, appearance_decay=decay))
    B, N = 64, 8
    rays, gt, u = dense_scene(dev, oracle, synthetic, B, N)
    opt = FusedAdam(net, lr=LR, max_grad_norm=float("inf") if kind == "guarded" else None)
    if kind == "masked":
        from nerf_simple_amd.utils.occupancy import OccupancyGrid
        bounds = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
        occ = OccupancyGrid.from_mask(torch.from_numpy(OM.ball_cells((33, 33, 33), bounds, 1.0)).to(dev), bounds, outside="empty")
        stepper = T.GraphedMaskedTrainStep(net, opt, B, N, occ, 1.0, **kw)
    elif kind == "device_rng":
        stepper = T.GraphedTrainStep(net, opt, B, N, device_rng=True, seed=40, **kw)
        return Checked(stepper, lambda s, decay: s.step(rays, gt, decay=decay))
    else:
        stepper = T.GraphedTrainStep(net, opt, B, N, **kw)
    return Checked(stepper, lambda s, decay: s.step(rays, gt, u=u, decay=decay))


@pytest.mark.parametrize("kind", KINDS)
def test_forty_graphed_steps(dev, oracle, synthetic, kind):
    """Forty steps under lr_decay_factor(5e-4, 1e-4, 40) with check_every=3 (whole-iteration graphs and A / B pairs both
    run; the 16-slot ring wraps twice).  After each: ``stepper.hyper`` is adam_model.scalars of the learning rate read in
    front of the step and of t, with t in words 6-7, bit for bit, and the ring's device counter is t; the update is
    nerf_amd_adam_step_hyper on clones taken in front of the step, the stepper's own stored gradient (so the dW atomics'
    order cannot enter) and a hyper vector the test built; the two images are a fresh pack of the new weights.  A guarded
    optimiser is limited to half the first measured norm from step 20 on and to half the last measured norm from step 30
    on (the rebuilt step uses the record's coef); a table stepper's second Adam passes the same checks
    and takes a new rate between steps 20 and 21."""
    from nerf_simple_amd.training import lr_decay_factor
    c = build(kind, dev, oracle, synthetic)
    s = c.stepper
    assert s.graph_ab is not None and s.check_every == 3
    decay = lr_decay_factor(5e-4, 1e-4, B2_STEPS)
    norm1, clipped, lr = None, 0, LR
    for k in range(1, B2_STEPS + 1):
        if kind == "guarded" and k == 20:
            c.opt.set_max_grad_norm(0.5 * norm1)
        if kind == "guarded" and k == 30:                             # by now the norm may lie below that limit: clip for sure
            c.opt.set_max_grad_norm(0.5 * float(s.grad_norm))
        if kind in TABLE_LR and k == 21:
            setattr(s, TABLE_LR[kind], 7e-4)
        loss = c.step(decay)
        lr *= decay
        assert c.opt.step_count == k and c.pg["lr"] == lr and bool(torch.isfinite(loss)), k
        if kind == "guarded":
            norm1 = norm1 or float(s.grad_norm)
            clipped += c.coef < 1.0
        if kind in TABLE_LR:
            assert c.a2.steps == k
            if k == 21:
                assert c.lr2 == 7e-4 and float(c.a2.hyper[0]) == float(np.float32(7e-4))
    if kind == "guarded":
        print(f"guarded: {clipped} of the steps from 20 on were clipped (half the first norm, {0.5 * norm1:.4g}, then half of step 29's)")
        assert c.opt.guard_stats()["skipped"] == 0 and c.opt.guard_stats()["clipped"] == clipped >= 1


# ---- B3: the jitter key across the wrap ---------------------------------------------------------------------------------------
def test_jitter_key_across_the_wrap(dev, golden, oracle, synthetic):
    """GraphedTrainStep(device_rng=True, seed=40, ray_id0=3 B), lr = 0: at steps 1, 16, 17, 32, 33 -- both sides of both
    wraps of the 16-slot ring -- ``stepper.ts`` is oracle.sample_ts of the counter RNG's uniforms under key 40 + t, bit for
    bit: the kernels form the positions with separately rounded fp32 operations from an exactly representable u, as the
    reference does on the CPU, and test_graphed_step_with_device_jitter allows the positions no ulp either."""
    import background_model as BM
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedTrainStep
    g = golden("train.npz")
    rays, gt, N = torch.from_numpy(g["rays"]).to(dev), torch.from_numpy(g["gt"]).to(dev), int(g["N"])
    B = rays.shape[0]
    net = make_net(dev, synthetic)
    stepper = GraphedTrainStep(net, FusedAdam(net, lr=0.0), B, N, device_rng=True, seed=40, ray_id0=3 * B)
    seen = []
    for t in range(1, 34):
        stepper.step(rays, gt)
        if t in (1, 16, 17, 32, 33):
            torch.cuda.synchronize()
            u = BM.jitter_uniforms(40 + t, 3 * B, B, N)
            u32 = torch.from_numpy(u.astype(np.float32))
            assert np.array_equal(u32.double().numpy(), u)             # 24-bit uniforms: exact in fp32
            want = oracle.sample_ts(u32)
            assert want.dtype == torch.float32 and same_bits(stepper.ts.cpu(), want), t
            assert int(stepper.hyper[6:8].view(torch.int64).item()) == t
            seen.append(stepper.ts.clone())
    assert not torch.equal(seen[0], seen[2]) and not torch.equal(seen[1], seen[3])     # slot 0 / slot 15 one wrap later


# ---- B4: interrupted bookkeeping is not silent ------------------------------------------------------------------------------
class Interrupted(Exception):
    pass


@pytest.mark.parametrize("kind,ring", (("plain", "_ring"), ("camera", "_ring"), ("camera", "_adam2.ring")))
def test_interrupted_bookkeeping(monkeypatch, dev, oracle, synthetic, kind, ring):
    """The ring's ``launched`` raises once -- a host exception behind an enqueued replay, as a KeyboardInterrupt there would
    be -- on a whole-iteration step (2) and on an A / B step (6).  The step behind each must run with exactly its own
    scalars and pass every B2 check, or raise a RuntimeError that names the desynchronisation; the checks then go on past
    the ring's wrap."""
    from nerf_simple_amd.training import lr_decay_factor
    c = build(kind, dev, oracle, synthetic)
    s = c.stepper
    target = s._ring if ring == "_ring" else s._adam2.ring
    real = target.launched
    decay = lr_decay_factor(5e-4, 1e-4, B2_STEPS)

    def once(dev_):
        monkeypatch.setattr(target, "launched", real)
        raise Interrupted("between the replay and the ring's bookkeeping")

    for k in range(1, 21):
        if k in (2, 6):
            monkeypatch.setattr(target, "launched", once)
            with pytest.raises(Interrupted):
                c.run(s, decay)
            torch.cuda.synchronize()
            assert target.launched == real and c.opt.step_count == k   # an attempted step: time passed
            continue
        c.snapshot()
        try:
            c.run(s, decay)
        except RuntimeError as e:
            assert "desynchron" in str(e) or "lockstep" in str(e), e    # loud is the other acceptable answer
            return
        c.check()
        assert c.opt.step_count == k
        if c.a2 is not None:
            assert c.a2.steps == k
