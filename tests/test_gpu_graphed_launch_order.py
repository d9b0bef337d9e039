"""The launch sequence of the four graphed training steps (training.GraphedTrainStep and its three subclasses; DESIGN.md
section 19): what each stepper enqueues, in which order, on which of its two streams and over how many points.

A recording proxy stands in for the object ``_lib.lib()`` returns.  It forwards every call and notes, for each launching
entry point of the step, (name, stream, point count); the stream is the entry point's last argument.  Constructing a
stepper enqueues its forward / backward sequence several times -- the warm-up, graph A, the whole-iteration graph -- and
its update (graph B, the whole-iteration graph): every copy must equal the list written out below, which restates the
class docstrings (one fork behind the last head, everything the dW products need besides dY on the side branch beside
the dX chain, the next batch's selection last on it).  ``step()`` replays graphs: it launches nothing of this by hand but
the selection that primes the first batch.

The lists are literal on purpose: they were written against the four separate implementations this sequence had, and hold
the one that replaced them to the same launches."""
import math

import numpy as np
import pytest
import torch

import occupancy_hierarchical_model as H
import occupancy_model as M

pytestmark = pytest.mark.gpu

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
R129 = (129, 129, 129)
B, N = 37, 65                   # ragged everywhere: no multiple of a tile, a wave or a mask word
NC, NF = 66, 65

FETCH, ADAM, SELECT = "nerf_amd_hyper_fetch", "nerf_amd_adam_step_hyper", "nerf_amd_select_rays"


def _at(i):
    return lambda a: int(a[i])


def _rows(i):
    return lambda a: int(a[i]) * int(a[i + 1])


# the point count of every launching entry point of the step: which of its arguments say how much work the launch is
COUNT = {
    FETCH: lambda a: None,
    "nerf_amd_mlp_forward_train": _rows(-3),                              # ..., B, N, stream
    "nerf_amd_volume_render_mse_backward": _rows(-3),                     # ..., B, N, stream
    "nerf_amd_volume_render_mse_backward_pdf": _rows(-4),                 # ..., B, Nc, Nf, stream
    "nerf_amd_sample_encode_bf16": _rows(-3),                             # ..., B, N, stream
    "nerf_amd_mlp_backward": _at(-2),                                     # ..., P, stream
    "nerf_amd_mlp_backward_e4m3": _at(-2),
    "nerf_amd_param_gradients_convert_e4m3": _at(-3),                     # ..., P, what, stream
    "nerf_amd_mse_loss": _at(-2),                                         # ..., n, stream
    "nerf_amd_param_gradients_begin": _at(-2),                            # ..., P, stream
    "nerf_amd_param_gradients_finish_bucket": _at(-3),                    # ..., P, bucket, stream
    "nerf_amd_param_gradients_finish_e4m3": _at(-3),
    "nerf_amd_occupancy_mark": _rows(-3),                                 # ..., B, N, stream
    "nerf_amd_occupancy_points_capped": _at(-4),                          # ..., C, B, N, stream
    "nerf_amd_mlp_forward_train_points": _at(-2),                         # ..., P, stream
    "nerf_amd_volume_render_masked_mse_backward": _at(-4),                # ..., C, B, N, stream
    "nerf_amd_volume_render_masked_mse_backward_pdf": _at(-5),            # ..., C, B, Nc, Nf, stream
    "nerf_amd_encode_points_bf16": _at(-2),                               # ..., P, stream
    SELECT: _at(4),                                                       # draws, seed, seed_mem, n, B, ...
    ADAM: _at(4),                                                         # flat, grads, m, v, n, hyper, stream
    "nerf_amd_pack_weights_train": lambda a: None,
}


class Recorder:
    """Stands in for the loaded library: forwards every call, notes the launches of COUNT."""

    def __init__(self, real):
        self._real, self.trace, self._wrapped = real, [], {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in COUNT:
            return fn
        if name not in self._wrapped:
            def call(*a, _fn=fn, _name=name):
                stream = getattr(a[-1], "value", a[-1]) or 0
                self.trace.append((_name, stream, COUNT[_name](a)))
                return _fn(*a)
            self._wrapped[name] = call
        return self._wrapped[name]

    def take(self):
        out, self.trace = self.trace, []
        return out


def sequences(trace):
    """The trace cut in front of every hyper fetch and every Adam launch; inside a piece a stream is 'main' if it is the
    stream of the piece's first launch and 'side' otherwise."""
    pieces = []
    for name, stream, count in trace:
        if name in (FETCH, ADAM) or not pieces:
            pieces.append([])
            main = stream
        pieces[-1].append((name, "main" if stream == main else "side", count))
    return pieces


# ---- the expected sequences, one readable list per stepper -------------------------------------------------------------
def dense(P, select):
    return ([(FETCH, "main", None),
             ("nerf_amd_mlp_forward_train", "main", P),
             ("nerf_amd_volume_render_mse_backward", "main", P),             # the head; the fork is recorded behind it
             ("nerf_amd_mlp_backward", "main", P),                           # the dX chain
             ("nerf_amd_sample_encode_bf16", "side", P),                     # beside it: the encoder rows first,
             ("nerf_amd_mse_loss", "side", 3 * B),                           # the loss value,
             ("nerf_amd_param_gradients_begin", "side", P)]                  # the zero fill + d_raw pack,
            + ([(SELECT, "side", B)] if select else [])                      # and last the next batch's selection
            + [("nerf_amd_param_gradients_finish_bucket", "main", P)])       # behind the join: the dW products


def dense_e4m3(P):
    return [(FETCH, "main", None),
            ("nerf_amd_mlp_forward_train", "main", P),
            ("nerf_amd_volume_render_mse_backward", "main", P),
            ("nerf_amd_mlp_backward_e4m3", "main", P),
            ("nerf_amd_sample_encode_bf16", "side", P),
            ("nerf_amd_param_gradients_convert_e4m3", "side", P),            # the encoder rows in 8 bits
            ("nerf_amd_mse_loss", "side", 3 * B),
            ("nerf_amd_param_gradients_begin", "side", P),
            ("nerf_amd_param_gradients_convert_e4m3", "side", P),            # the packed d_raw likewise
            ("nerf_amd_param_gradients_finish_e4m3", "main", P)]


def masked(P, C, select):
    return ([(FETCH, "main", None),
             ("nerf_amd_occupancy_mark", "main", P),
             ("nerf_amd_occupancy_points_capped", "main", C),
             ("nerf_amd_mlp_forward_train_points", "main", C),
             ("nerf_amd_volume_render_masked_mse_backward", "main", C),
             ("nerf_amd_mlp_backward", "main", C),
             ("nerf_amd_encode_points_bf16", "side", C),
             ("nerf_amd_mse_loss", "side", 3 * B),
             ("nerf_amd_param_gradients_begin", "side", C)]
            + ([(SELECT, "side", B)] if select else [])
            + [("nerf_amd_param_gradients_finish_bucket", "main", C)])


def pair(Pc, Pf, select):
    return ([(FETCH, "main", None),
             ("nerf_amd_mlp_forward_train", "main", Pc),
             ("nerf_amd_volume_render_mse_backward_pdf", "main", Pc),        # the coarse head writes ts_f
             ("nerf_amd_mlp_forward_train", "main", Pf),
             ("nerf_amd_volume_render_mse_backward", "main", Pf),            # the fork is behind BOTH heads
             ("nerf_amd_mlp_backward", "main", Pc),
             ("nerf_amd_mlp_backward", "main", Pf),
             ("nerf_amd_sample_encode_bf16", "side", Pc),
             ("nerf_amd_sample_encode_bf16", "side", Pf),
             ("nerf_amd_mse_loss", "side", 3 * B),
             ("nerf_amd_param_gradients_begin", "side", Pc),
             ("nerf_amd_mse_loss", "side", 3 * B),
             ("nerf_amd_param_gradients_begin", "side", Pf)]
            + ([(SELECT, "side", B)] if select else [])
            + [("nerf_amd_param_gradients_finish_bucket", "main", Pc),
               ("nerf_amd_param_gradients_finish_bucket", "main", Pf)])


def masked_pair(Pc, Pf, Cc, Cf, select):
    return ([(FETCH, "main", None),
             ("nerf_amd_occupancy_mark", "main", Pc),
             ("nerf_amd_occupancy_points_capped", "main", Cc),
             ("nerf_amd_mlp_forward_train_points", "main", Cc),
             ("nerf_amd_volume_render_masked_mse_backward_pdf", "main", Cc),
             ("nerf_amd_occupancy_mark", "main", Pf),                        # on ts_f: behind the coarse head
             ("nerf_amd_occupancy_points_capped", "main", Cf),
             ("nerf_amd_mlp_forward_train_points", "main", Cf),
             ("nerf_amd_volume_render_masked_mse_backward", "main", Cf),
             ("nerf_amd_mlp_backward", "main", Cc),
             ("nerf_amd_mlp_backward", "main", Cf),
             ("nerf_amd_encode_points_bf16", "side", Cc),
             ("nerf_amd_encode_points_bf16", "side", Cf),
             ("nerf_amd_mse_loss", "side", 3 * B),
             ("nerf_amd_param_gradients_begin", "side", Cc),
             ("nerf_amd_mse_loss", "side", 3 * B),
             ("nerf_amd_param_gradients_begin", "side", Cf)]
            + ([(SELECT, "side", B)] if select else [])
            + [("nerf_amd_param_gradients_finish_bucket", "main", Cc),
               ("nerf_amd_param_gradients_finish_bucket", "main", Cf)])


def update(n_params, n_nets):
    return [(ADAM, "main", n_params)] + [("nerf_amd_pack_weights_train", "main", None)] * n_nets


# ---- the harness -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def inputs(dev, oracle, synthetic):
    """rays / gt / jitter of the ragged pair shape (shared by the dense cases: u = the first N columns' worth of a draw),
    a ray table for ``rays_from`` and the ball grid of the masked tests"""
    from nerf_simple_amd.utils.dataload import RayGenerator
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    rays, gt, u_c, u_f = (t.to(dev) for t in H.pair_inputs(oracle, synthetic, B, NC, NF))
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(3)).to(dev)
    pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, -30, 0))).float()
    table = oracle.camera_rays(pose, [10, 10, synthetic.focal_from_fov(10)]).contiguous()
    rg = RayGenerator.from_tables(table, torch.rand(table.shape[0], 3, generator=torch.Generator().manual_seed(4)), device=dev)
    occ = OccupancyGrid.from_mask(torch.from_numpy(M.ball_cells(R129, BOUNDS, 1.0)).to(dev), BOUNDS, outside="empty")
    return dict(rays=rays, gt=gt, u=u, u_c=u_c, u_f=u_f, rg=rg, occ=occ)


def make_nets(dev, synthetic, n):
    from nerf_simple_amd.utils.nets import Nerf
    nets = []
    for seed in range(n):
        net = Nerf(precision="bf16").to(dev)
        net.load_state_dict(synthetic.synthetic_state_dict(seed, "default"))
        nets.append(net)
    return nets


def run_case(monkeypatch, dev, synthetic, n_nets, build, step, want, warmup_tail, select):
    """build(nets, opt) -> stepper under the recorder; step(stepper) runs one iteration.  ``want`` is the forward / backward
    sequence, ``warmup_tail`` what the warm-up enqueues behind its copy of it (the dense stepper warms the head-gradient
    launch of its two-bucket form up too)."""
    from nerf_simple_amd import _lib
    from nerf_simple_amd.optim import FusedAdam
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    nets = make_nets(dev, synthetic, n_nets)
    opt = FusedAdam(nets if n_nets > 1 else nets[0], lr=0.0)
    rec.take()
    stepper = build(nets, opt)
    got = sequences(rec.take())
    upd = update(opt.flat.numel(), n_nets)
    # one process, no exchange: the warm-up, graph A, graph B, then the whole iteration as one graph
    assert stepper.graph_ab is not None and stepper.graph_a2 is None
    names = ["warm-up", "graph A", "graph B", "graph AB: forward / backward", "graph AB: update"]
    wanted = [want + warmup_tail, want, upd, want, upd]
    assert len(got) == len(wanted), [p[0][0] for p in got]
    for name, g, w in zip(names, got, wanted):
        assert g == w, (name, [x for x in zip(g, w) if x[0] != x[1]][:3], len(g), len(w))
    assert got[1] == got[3] and got[0][:len(want)] == got[1]               # the warm-up and the captures are one sequence
    loss = step(stepper)
    eager = rec.take()
    # step() replays: by hand it launches the selection that primes the first batch, on the current stream, and nothing else
    assert [(n, c) for n, _, c in eager] == ([(SELECT, B)] if select else []), eager
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    return stepper


JITTER = ("u", "device_rng+rays_from")


def jitter_kw(mode, inputs):
    return dict(device_rng=True, seed=11, rays_from=inputs["rg"]) if mode != "u" else {}


@pytest.mark.parametrize("variant", JITTER + ("e4m3",))
def test_dense_step(monkeypatch, dev, synthetic, inputs, variant):
    from nerf_simple_amd.training import GraphedTrainStep
    P, select = B * N, variant == JITTER[1]
    kw = dict(storage="e4m3") if variant == "e4m3" else jitter_kw(variant, inputs)
    want = dense_e4m3(P) if variant == "e4m3" else dense(P, select)
    tail = [(want[-1][0], "main", P)]                      # _head_gradients: the second launch of the bucketed form
    run_case(monkeypatch, dev, synthetic, 1, lambda nets, opt: GraphedTrainStep(nets[0], opt, B, N, **kw),
             lambda s: s.step() if select else s.step(inputs["rays"], inputs["gt"], u=inputs["u"]), want, tail, select)


@pytest.mark.parametrize("variant", JITTER)
def test_masked_step(monkeypatch, dev, synthetic, inputs, variant):
    from nerf_simple_amd.training import GraphedMaskedTrainStep
    select = variant == JITTER[1]
    C = math.ceil(0.5 * B * N)
    s = run_case(monkeypatch, dev, synthetic, 1,
                 lambda nets, opt: GraphedMaskedTrainStep(nets[0], opt, B, N, inputs["occ"], 0.5, **jitter_kw(variant, inputs)),
                 lambda s: s.step() if select else s.step(inputs["rays"], inputs["gt"], u=inputs["u"]),
                 masked(B * N, C, select), [], select)
    assert s.capacity == C


@pytest.mark.parametrize("variant", JITTER)
def test_pair_step(monkeypatch, dev, synthetic, inputs, variant):
    from nerf_simple_amd.training import GraphedHierarchicalTrainStep
    select = variant == JITTER[1]
    run_case(monkeypatch, dev, synthetic, 2,
             lambda nets, opt: GraphedHierarchicalTrainStep(nets[0], nets[1], opt, B, NC, NF, **jitter_kw(variant, inputs)),
             lambda s: s.step() if select else s.step(inputs["rays"], inputs["gt"], u_c=inputs["u_c"], u_f=inputs["u_f"]),
             pair(B * NC, B * (NC + NF), select), [], select)


@pytest.mark.parametrize("variant", JITTER)
def test_masked_pair_step(monkeypatch, dev, synthetic, inputs, variant):
    from nerf_simple_amd.training import GraphedMaskedHierarchicalTrainStep
    select = variant == JITTER[1]
    Pc, Pf = B * NC, B * (NC + NF)
    Cc, Cf = math.ceil(0.5 * Pc), math.ceil(0.5 * Pf)
    s = run_case(monkeypatch, dev, synthetic, 2,
                 lambda nets, opt: GraphedMaskedHierarchicalTrainStep(nets[0], nets[1], opt, B, NC, NF, inputs["occ"], (0.5, 0.5),
                                                                      **jitter_kw(variant, inputs)),
                 lambda s: s.step() if select else s.step(inputs["rays"], inputs["gt"], u_c=inputs["u_c"], u_f=inputs["u_f"]),
                 masked_pair(Pc, Pf, Cc, Cf, select), [], select)
    assert s.capacity == (Cc, Cf)
