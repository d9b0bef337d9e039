"""The gradient guard on the device (definition: include/nerf_amd.h, model: tests/grad_guard_model.py):
the norm kernel alone, the skip rule, the definition chain norm -> coef -> coef g -> nerf_amd_adam_step_hyper bit for bit
through eager FusedAdam and inside the captured graphs, a withheld step that leaves nothing behind, the launch sequences
with and without the guard, the two refusing steppers and the asynchronous watch.

Sizes: the reduction's partition gives element i to thread i mod 262,144 (256 workgroups of 1,024 threads), four elements
of a thread per loop round -- so the sizes sit on both sides of a wave (64), a workgroup's share (1,024), the whole grid
(262,144) and a loop round (1,048,576), beside the small ones and the network's 595,844."""
import warnings

import numpy as np
import pytest
import torch

import grad_guard_model as G
import occupancy_hierarchical_model as H

pytestmark = pytest.mark.gpu

N_NET = 595844
GUARD, GUARDED, ADAM, PACK = ("nerf_amd_grad_guard", "nerf_amd_adam_step_guarded", "nerf_amd_adam_step_hyper",
                              "nerf_amd_pack_weights_train")


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


def new_record(dev, max_norm):
    rec = torch.zeros(8, dtype=torch.float32, device=dev)
    rec[0] = max_norm
    return rec


def run_guard(g, rec):
    """nerf_amd_grad_guard on ``g`` into ``rec``; the record on the host as (float32 view, int32 view)."""
    from nerf_simple_amd import _lib
    n = g.numel()
    ws = torch.empty(int(_lib.lib().nerf_amd_grad_guard_workspace_bytes(n)), dtype=torch.uint8, device=rec.device)
    _lib.launch("nerf_amd_grad_guard", g if n else None, n, ws, rec, dev=rec.device)
    h = rec.cpu()
    return h.numpy().copy(), h.view(torch.int32).numpy().copy()


def make_net(dev, synthetic, seed=0):
    from nerf_simple_amd.utils.nets import Nerf
    net = Nerf(precision="bf16").to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(seed, "default"))
    return net


def hand_gradients(net, dev, seed, scale=1.0):
    """Gradients set by hand (as test_fused_adam_matches_torch does: |g| spans eps .. 1), and the flat vector they form."""
    gen = torch.Generator().manual_seed(seed)
    for prm in net.parameters():
        mag = torch.pow(10.0, torch.rand(prm.shape, generator=gen) * 8 - 8)
        prm.grad = (torch.randn(prm.shape, generator=gen) * mag * scale).to(dev)
    return torch.cat([p.grad.reshape(-1) for p in net.parameters()])


# ---- 1. the norm kernel alone ------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 262143, 262144, 262145, N_NET, 1048575, 1048576, 1048577)


@pytest.mark.parametrize("n", SIZES)
def test_norm_kernel(dev, n):
    """|norm - fl32(model)| <= 1 fp32 ulp: the squares are exact in double and the double sum's relative error is at most
    n 2^-53 (< 2^-32 here), far inside half an fp32 ulp, so only the final rounding can differ, at a tie -- derived, not
    observed.  Two runs write the same bytes; the limit is far away, so coef is 1 and nothing is skipped or clipped."""
    gen = torch.Generator().manual_seed(100 + n % 997)
    g_host = torch.randn(n, generator=gen) * torch.pow(10.0, torch.rand(n, generator=gen) * 6 - 6)
    g = g_host.to(dev)
    rec = new_record(dev, float("inf"))
    f, w = run_guard(g, rec)
    want = G.norm32(g_host.numpy())
    print(f"n={n} norm={f[1]!r} model={want!r}")
    assert abs(float(f[1]) - float(want)) <= G.ulp(want), (n, f[1], want)
    assert (n > 0) == (f[1] > 0)
    assert f[0] == np.inf and f[2] == 1.0 and list(w[3:]) == [0, 1, 0, 0, 0]
    rec2 = new_record(dev, float("inf"))
    f2, w2 = run_guard(g, rec2)
    assert np.array_equal(w, w2)                                     # the same bytes
    f3, w3 = run_guard(g, rec)                                       # the same record again: only the step counter moves
    assert np.array_equal(w3[:4], w[:4]) and list(w3[4:]) == [2, 0, 0, 0]


@pytest.mark.parametrize("n", (257, N_NET))
def test_norm_kernel_ranges(dev, n):
    """Gradients an fp32 accumulator could not hold: 3e19 everywhere (the squares overflow fp32) gives a finite norm and no
    skip; 1e-30 everywhere (the squares underflow fp32) gives a non-zero norm.  Both within 1 ulp of the model."""
    for value in (3e19, 1e-30):
        g = torch.full((n,), value, dtype=torch.float32, device=dev)
        f, w = run_guard(g, new_record(dev, float("inf")))
        want = G.norm32(np.full(n, value, np.float32))
        print(f"n={n} value={value} norm={f[1]!r} model={want!r}")
        assert np.isfinite(f[1]) and f[1] > 0 and abs(float(f[1]) - float(want)) <= G.ulp(want)
        assert f[2] == 1.0 and list(w[3:]) == [0, 1, 0, 0, 0]


def test_coef_rule_and_clipped_counter(dev):
    """coef is the model's fp32 rule formed from the DEVICE's norm, bit for bit, on both sides of the limit; the clipped
    counter counts coef < 1."""
    g = torch.randn(5000, generator=torch.Generator().manual_seed(3)).to(dev)
    rec = new_record(dev, 1.0)
    clipped = 0
    norm = float(G.norm32(g.cpu().numpy()))                            # about sqrt(5000)
    for max_norm in (1.0, 1e-3, 1e4, norm * (1 - 1e-3), norm * (1 + 1e-3), float("inf"), 1e-30):
        rec[0] = max_norm
        f, w = run_guard(g, rec)
        want = G.coef(max_norm, f[1])
        assert f[2].tobytes() == np.float32(want).tobytes(), (max_norm, f[2], want)
        clipped += bool(want < 1)
        assert w[3] == 0 and w[5] == 0 and w[6] == clipped
    assert clipped == 4


# ---- 2. the skip rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1500, N_NET))
def test_skip_rule(dev, n):
    """One NaN, one +inf, one -inf in turn at element 0, element n - 1, an element of the last workgroup-share's ragged tail,
    and one element in each of two different workgroups: skip is set, coef is 0, the skipped counter rises by one."""
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(5)).to(dev)
    tail = (n // 1024) * 1024 + (n % 1024) // 2
    places = ((0,), (n - 1,), (tail,), (5, 1024 + 5))
    rec = new_record(dev, 1.0)
    skipped = 0
    for bad in (float("nan"), float("inf"), -float("inf")):
        for where in places:
            g = g0.clone()
            g[list(where)] = bad
            f, w = run_guard(g, rec)
            skipped += 1
            assert w[3] == 1 and f[2] == 0.0 and w[5] == skipped and w[6] == 0, (bad, where, f, w)
            assert not np.isfinite(f[1])
    f, w = run_guard(g0, rec)                                        # a clean gradient behind them: the verdict is this step's
    assert w[3] == 0 and 0 < f[2] < 1 and list(w[4:7]) == [skipped + 1, skipped, 1]


def test_skip_when_the_norm_leaves_fp32(dev):
    g = torch.full((N_NET,), 3e38, dtype=torch.float32, device=dev)
    f, w = run_guard(g, new_record(dev, float("inf")))
    assert np.isinf(f[1]) and w[3] == 1 and f[2] == 0.0 and list(w[4:7]) == [1, 1, 0]


# ---- 3. the chain, bit for bit, through eager FusedAdam --------------------------------------------------------------
def test_eager_chain_bit_for_bit(dev, synthetic):
    """One optimiser, three steps: a limit of half the gradient's norm (clips), inf (the plain update, bit for bit) and a
    limit above the norm (coef exactly 1).  Each step is rebuilt from clones taken in front of it: the model's coef from the
    device's norm, g * coef in torch fp32, nerf_amd_adam_step_hyper with the step's own six scalars."""
    from nerf_simple_amd import _lib
    from nerf_simple_amd.optim import FusedAdam
    net = make_net(dev, synthetic)
    opt = FusedAdam(net, lr=5e-4, max_grad_norm=float("inf"))
    assert opt.guard.shape == (8,) and opt.grad_norm.dim() == 0 and opt.grad_norm.data_ptr() == opt.guard.data_ptr() + 4
    n = opt.flat.numel()
    for k, limit in enumerate(("half", float("inf"), "double")):
        g = hand_gradients(net, dev, 11 + k)
        norm = float(G.norm32(g.cpu().numpy()))
        max_norm = {"half": 0.5 * norm, "double": 2.0 * norm}.get(limit, limit)
        opt.set_max_grad_norm(max_norm)
        before = [t.clone() for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq)]
        start = [t.clone() for t in before]
        opt.step()
        rec = opt.guard.cpu().numpy()
        stats = opt.guard_stats()
        assert abs(float(rec[1]) - norm) <= G.ulp(norm) and stats["norm"] == float(rec[1]) and not stats["skipped_last"]
        want = G.coef(max_norm, rec[1])
        assert rec[2].tobytes() == np.float32(want).tobytes(), (limit, rec[2], want)
        assert (want < 1) == (limit == "half") and (limit == "half" or want == 1)
        assert (stats["steps"], stats["skipped"], stats["clipped"]) == (k + 1, 0, 1) and opt.step_count == k + 1
        g2 = g if want == 1 else g * float(want)
        assert g2.dtype == torch.float32
        _lib.launch("nerf_amd_adam_step_hyper", before[0], g2, before[1], before[2], n, opt._hyper, dev=dev)
        for got, ref, name in zip((opt.flat, opt.exp_avg, opt.exp_avg_sq), before, ("params", "exp_avg", "exp_avg_sq")):
            assert same_bits(got, ref), (limit, name)
        if limit != "half":
            # ... and that is today's update: what the unguarded FusedAdam.step launches on the unscaled gradient
            _lib.launch("nerf_amd_adam_step", start[0], g, start[1], start[2], n, 5e-4, 0.9, 0.999, 1e-8, k + 1, dev=dev)
            for got, ref, name in zip((opt.flat, opt.exp_avg, opt.exp_avg_sq), start, ("params", "exp_avg", "exp_avg_sq")):
                assert same_bits(got, ref), (limit, "plain", name)
    assert float(opt.grad_norm) == opt.guard_stats()["norm"]


# ---- 4. a withheld step leaves nothing behind ----------------------------------------------------------------------------
def test_withheld_step_leaves_nothing_behind(dev, synthetic):
    """A NaN in the gradient: parameters, both moments and both packed training images are byte-equal before and after; the
    next clean step is the plain update with step count 2's scalars (time passed on the withheld step)."""
    from nerf_simple_amd import _lib
    from nerf_simple_amd.optim import FusedAdam
    net = make_net(dev, synthetic)
    opt = FusedAdam(net, lr=5e-4, max_grad_norm=float("inf"))
    images = [net.packed_weights(_lib.BF16), net.packed_weights(_lib.BF16_BWD)]
    hand_gradients(net, dev, 21)
    opt.step()                                                       # a clean step first: moments that are not zero
    state = (opt.flat, opt.exp_avg, opt.exp_avg_sq, *images)
    before = [t.clone() for t in state]
    hand_gradients(net, dev, 22)
    list(net.parameters())[3].grad.view(-1)[17] = float("nan")
    opt.step()
    stats = opt.guard_stats()
    assert stats["skipped_last"] and stats["coef"] == 0.0 and np.isnan(stats["norm"])
    assert (stats["steps"], stats["skipped"], stats["clipped"]) == (2, 1, 0) and opt.step_count == 2
    assert net.packed_weights(_lib.BF16) is images[0] and net.packed_weights(_lib.BF16_BWD) is images[1]
    for got, ref, name in zip(state, before, ("params", "exp_avg", "exp_avg_sq", "forward image", "backward image")):
        assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8)), name
    g = hand_gradients(net, dev, 23)
    opt.step()
    assert not opt.guard_stats()["skipped_last"] and opt.step_count == 3
    _lib.launch("nerf_amd_adam_step", before[0], g, before[1], before[2], opt.flat.numel(), 5e-4, 0.9, 0.999, 1e-8, 3, dev=dev)
    for got, ref, name in zip(state[:3], before, ("params", "exp_avg", "exp_avg_sq")):
        assert same_bits(got, ref), name
    assert not torch.equal(images[0], before[3])                     # the clean step re-packed new weights


# ---- 5. inside the graphs ---------------------------------------------------------------------------------------------
def rebuild_step(stepper, before):
    """The definition chain on the clones ``before`` from what the replay left in the stepper's buffers; the coef used."""
    from nerf_simple_amd import _lib
    opt = stepper.opt
    rec = opt.guard.cpu().numpy()
    want = G.coef(rec[0], rec[1])
    assert rec[2].tobytes() == np.float32(want).tobytes(), (rec, want)
    assert abs(float(rec[1]) - float(G.norm32(stepper.grads.cpu().numpy()))) <= G.ulp(rec[1])
    g2 = stepper.grads if want == 1 else stepper.grads * float(want)
    _lib.launch("nerf_amd_adam_step_hyper", before[0], g2, before[1], before[2], opt.flat.numel(), stepper.hyper, dev=stepper.dev)
    for got, ref, name in zip((opt.flat, opt.exp_avg, opt.exp_avg_sq), before, ("params", "exp_avg", "exp_avg_sq")):
        assert same_bits(got, ref), name
    return float(want)


def test_inside_the_graphs(dev, oracle, synthetic):
    """GraphedTrainStep at 64 rays x 8 samples: three steps with max_grad_norm = inf, three under half the first step's
    measured norm (set in place between replays: no re-capture), each rebuilt from ``stepper.grads`` within the one stepper
    (so the dW products' summation order cannot enter); check_every=2 runs both the whole-iteration graph and the A / B
    pair.  Then a batch whose gt holds one NaN -- a value, not a fault: the step is withheld, the following one trains."""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedTrainStep
    B, N = 64, 8
    rays, gt, u, _ = (t.to(dev) for t in H.pair_inputs(oracle, synthetic, B, N, 4))
    net = make_net(dev, synthetic)
    opt = FusedAdam(net, lr=5e-4, max_grad_norm=float("inf"))
    stepper = GraphedTrainStep(net, opt, B, N, check_every=2)
    assert stepper.graph_ab is not None
    assert opt.guard_stats()["steps"] == 0                           # the captures executed nothing
    assert stepper.grad_norm.data_ptr() == opt.guard.data_ptr() + 4
    state = (opt.flat, opt.exp_avg, opt.exp_avg_sq)
    norm1 = None
    for k in range(6):
        if k == 3:
            opt.set_max_grad_norm(0.5 * norm1)
        before = [t.clone() for t in state]
        loss = stepper.step(rays, gt, u=u)
        coef = rebuild_step(stepper, before)
        norm1 = norm1 or float(stepper.grad_norm)
        assert (coef == 1.0) == (k < 3), (k, coef)
        assert bool(torch.isfinite(loss))
    stats = opt.guard_stats()
    assert (stats["steps"], stats["skipped"], stats["clipped"]) == (6, 0, 3) and opt.step_count == 6
    bad_gt = gt.clone()
    bad_gt[B // 2, 1] = float("nan")
    before = [t.clone() for t in state]
    images = [b.clone() for _, _, bufs in stepper._images for b in bufs]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # the watch's report is test_guard_watch's subject
        stepper.step(rays, bad_gt, u=u)
        stats = opt.guard_stats()
        assert stats["skipped_last"] and (stats["steps"], stats["skipped"], stats["clipped"]) == (7, 1, 3)
        for got, ref in zip(state, before):
            assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8))
        for got, ref in zip([b for _, _, bufs in stepper._images for b in bufs], images):
            assert torch.equal(got, ref)
        loss = stepper.step(rays, gt, u=u)                           # the following clean step trains
    held = before[0].clone()                                             # (rebuild_step updates the clones in place)
    rebuild_step(stepper, before)
    assert bool(torch.isfinite(loss)) and not same_bits(opt.flat, held) and bool(torch.isfinite(opt.flat).all())
    assert opt.guard_stats()["skipped"] == 1 and opt.step_count == 8


def test_pair_has_one_norm(dev, oracle, synthetic):
    """GraphedHierarchicalTrainStep at 32 x (8 + 8): ONE norm over both networks' gradients, as clip_grad_norm_ over all
    parameters gives; the step is the chain on the whole flat vector."""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedHierarchicalTrainStep
    B, Nc, Nf = 32, 8, 8
    rays, gt, u_c, u_f = (t.to(dev) for t in H.pair_inputs(oracle, synthetic, B, Nc, Nf))
    nets = [make_net(dev, synthetic, s) for s in (0, 1)]
    opt = FusedAdam(nets, lr=5e-4, max_grad_norm=float("inf"))
    stepper = GraphedHierarchicalTrainStep(nets[0], nets[1], opt, B, Nc, Nf, check_every=0)
    assert stepper.grads.numel() == 2 * N_NET
    for k in range(2):
        if k == 1:
            opt.set_max_grad_norm(0.25 * float(stepper.grad_norm))
        before = [t.clone() for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq)]
        stepper.step(rays, gt, u_c=u_c, u_f=u_f)
        g = stepper.grads.cpu().numpy()
        whole, halves = G.norm32(g), [float(G.norm32(h)) for h in (g[:N_NET], g[N_NET:])]
        assert min(halves) > 0 and abs(float(stepper.grad_norm) - float(whole)) <= G.ulp(whole)
        assert float(whole) > max(halves)                            # neither network's own norm
        assert (rebuild_step(stepper, before) < 1) == (k == 1)


# ---- 6. off means off --------------------------------------------------------------------------------------------------
class Recorder:
    """Stands in for the loaded library: forwards every call and notes (name, element count) of the update's launches and
    the bare name of every other launch (an entry point whose last argument is a stream that is given)."""

    def __init__(self, real):
        self._real, self.trace = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("nerf_amd_") or name.endswith("_bytes") or not fn.argtypes or len(fn.argtypes) < 2:
            return fn

        def call(*a):
            if name in (GUARD, GUARDED, ADAM):
                self.trace.append((name, int(a[1] if name == GUARD else a[4])))
            elif getattr(a[-1], "value", a[-1]):                      # a launch on a stream of the stepper's
                self.trace.append((name, None))
            return fn(*a)
        return call


@pytest.mark.parametrize("kind", ("dense", "pair"))
def test_off_means_off(monkeypatch, dev, oracle, synthetic, kind):
    """A stepper on FusedAdam(net) launches what it launched (Adam, re-pack: graph B and the whole-iteration graph); on a
    guarded optimiser the SAME sequence with nerf_amd_grad_guard, nerf_amd_adam_step_guarded in Adam's place."""
    from nerf_simple_amd import _lib
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedHierarchicalTrainStep, GraphedTrainStep
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    traces = []
    for max_norm in (None, 1.0):
        nets = [make_net(dev, synthetic, s) for s in range(2 if kind == "pair" else 1)]
        opt = FusedAdam(nets if kind == "pair" else nets[0], lr=0.0, max_grad_norm=max_norm)
        rec.trace = []
        if kind == "pair":
            stepper = GraphedHierarchicalTrainStep(nets[0], nets[1], opt, 32, 8, 8)
        else:
            stepper = GraphedTrainStep(nets[0], opt, 64, 8)
        assert stepper.graph_ab is not None
        traces.append(rec.trace)
    plain, guarded = traces
    n, packs = opt.flat.numel(), [(PACK, None)] * len(nets)
    update = [t for t in plain if t[0] in (GUARD, GUARDED, ADAM, PACK)]
    assert update == ([(ADAM, n)] + packs) * 2                       # graph B, then the tail of the whole-iteration graph
    assert [t for t in guarded if t[0] in (GUARD, GUARDED, ADAM, PACK)] == ([(GUARD, n), (GUARDED, n)] + packs) * 2
    swapped = []
    for t in plain:
        swapped += [(GUARD, n), (GUARDED, n)] if t[0] == ADAM else [t]
    assert guarded == swapped and len(plain) > 20                    # everything else launches exactly as it did


# ---- 7. refusals and the watch -----------------------------------------------------------------------------------------
def test_table_steppers_refuse_a_guarded_optimizer(dev, oracle, synthetic):
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedAppearanceTrainStep, GraphedCameraTrainStep
    from nerf_simple_amd.utils.appearance import AppearanceCorrection
    from nerf_simple_amd.utils.cameras import CameraRefinement
    from nerf_simple_amd.utils.dataload import RayGenerator
    M, side, B, N = 3, 5, 37, 8
    cam = [side, side, synthetic.focal_from_fov(side)]
    colours = torch.rand(M, side, side, 3, generator=torch.Generator().manual_seed(5)).numpy()
    poses = [np.asarray(oracle.spherical_to_pose(4, -30 - 5 * m, 90 * m), dtype=np.float32) for m in range(M)]
    table = RayGenerator.from_samples({"train": [{"img": im, "transform": p} for im, p in zip(colours, poses)]}, cam, dev)
    net = make_net(dev, synthetic)
    opt = FusedAdam(net, max_grad_norm=1.0)
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        GraphedCameraTrainStep(net, opt, B, N, CameraRefinement.from_ray_generator(table), rays_from=table, device_rng=True)
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        GraphedAppearanceTrainStep(net, opt, B, N, AppearanceCorrection.from_ray_generator(table), rays_from=table, device_rng=True)


def test_guard_watch_warns_once(dev, oracle, synthetic):
    """check_every=1 samples every step: after a withheld step has completed, the next ``step`` warns once, naming one step
    withheld up to that step; the steps behind it say nothing."""
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedTrainStep
    B, N = 64, 8
    rays, gt, u, _ = (t.to(dev) for t in H.pair_inputs(oracle, synthetic, B, N, 4))
    net = make_net(dev, synthetic)
    opt = FusedAdam(net, lr=5e-4, max_grad_norm=1.0)
    stepper = GraphedTrainStep(net, opt, B, N, check_every=1)
    bad_gt = gt.clone()
    bad_gt[0, 0] = float("nan")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        stepper.step(rays, gt, u=u)
        stepper.step(rays, bad_gt, u=u)                              # step 2 is withheld
        torch.cuda.synchronize()
        assert not [w for w in seen if issubclass(w.category, RuntimeWarning)]
        stepper.step(rays, gt, u=u)                                  # ... and reported here
        torch.cuda.synchronize()
        stepper.step(rays, gt, u=u)
        torch.cuda.synchronize()
        stepper.step(rays, gt, u=u)
    mine = [str(w.message) for w in seen if issubclass(w.category, RuntimeWarning)]
    assert len(mine) == 1 and "withheld 1 training step up to step 2" in mine[0], mine
    assert opt.guard_stats()["skipped"] == 1 and bool(torch.isfinite(opt.flat).all())
