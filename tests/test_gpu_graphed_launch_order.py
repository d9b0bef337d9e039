"""The launch sequence of the graphed training steps (training.GraphedTrainStep and its subclasses):
what each stepper enqueues, in which order, on which of its two streams and over how many points.

A recording proxy stands in for the object ``_lib.lib()`` returns.  It forwards every call and notes, for each launching
entry point of the step, (name, stream, point count); the stream is the entry point's last argument.  Constructing a
stepper enqueues its forward / backward sequence several times -- the warm-up, graph A, the whole-iteration graph -- and
its update (graph B, the whole-iteration graph): every copy must equal the list written out below, which restates the
class docstrings (one fork behind the last head, everything the dW products need besides dY on the side branch beside
the dX chain, the next batch's selection last on it).  ``step()`` replays graphs: it launches nothing of this by hand but
the selection that primes the first batch.

The lists are literal on purpose: they were written against the four separate implementations this sequence had, and hold
the one that replaced them to the same launches.  The lists of the dense step's controls, the two guided steppers and the
two steppers with a per-image table (cameras, appearance) were written the same way, against the steppers as each of them
carried its own copy of the second Adam and of the u_c / u_f handling, in front of the change that folded those copies."""
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
    "nerf_amd_volume_render_mse_backward_bg": _rows(-3),                  # ..., B, N, stream
    "nerf_amd_volume_render_mse_backward_dist": _rows(-3),
    "nerf_amd_volume_render_mse_backward_affine": _rows(-3),
    "nerf_amd_sum_f32": _at(-2),                                          # x, out, n, stream
    "nerf_amd_sample_pdf_volume": _rows(-4),                              # ..., B, Nc, Nf, stream: the coarse positions
    "nerf_amd_sample_pdf_volume_masked": _rows(-4),
    "nerf_amd_camera_rays": _at(-3),                                      # ..., B, M, stream
    "nerf_amd_camera_rays_backward": _at(-3),
    "nerf_amd_input_gradients": _at(-3),                                  # ..., P, N, stream
    "nerf_amd_appearance_gather": _at(-3),                                # ..., B, M, stream
    "nerf_amd_appearance_reduce": _at(-3),
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


def dense_controls(P, select):
    return ([(FETCH, "main", None),
             ("nerf_amd_mlp_forward_train", "main", P),
             ("nerf_amd_volume_render_mse_backward_bg", "main", P),          # the head behind the background, noise on sigma
             ("nerf_amd_mlp_backward", "main", P),
             ("nerf_amd_sample_encode_bf16", "side", P),
             ("nerf_amd_mse_loss", "side", 3 * B),
             ("nerf_amd_param_gradients_begin", "side", P)]
            + ([(SELECT, "side", B)] if select else [])
            + [("nerf_amd_param_gradients_finish_bucket", "main", P)])


def dense_distortion(P, select):
    return ([(FETCH, "main", None),
             ("nerf_amd_mlp_forward_train", "main", P),
             ("nerf_amd_volume_render_mse_backward_dist", "main", P),        # the head with the term beside the MSE
             ("nerf_amd_mlp_backward", "main", P),
             ("nerf_amd_sample_encode_bf16", "side", P),
             ("nerf_amd_mse_loss", "side", 3 * B),
             ("nerf_amd_param_gradients_begin", "side", P),
             ("nerf_amd_sum_f32", "side", B)]                                # the per-ray values of the term, summed
            + ([(SELECT, "side", B)] if select else [])
            + [("nerf_amd_param_gradients_finish_bucket", "main", P)])


def guided(Pc, P, select):
    return ([(FETCH, "main", None),
             ("nerf_amd_sample_pdf_volume", "main", Pc),                     # the placement, between the fetch and the forward
             ("nerf_amd_mlp_forward_train", "main", P),
             ("nerf_amd_volume_render_mse_backward", "main", P),
             ("nerf_amd_mlp_backward", "main", P),
             ("nerf_amd_sample_encode_bf16", "side", P),
             ("nerf_amd_mse_loss", "side", 3 * B),
             ("nerf_amd_param_gradients_begin", "side", P)]
            + ([(SELECT, "side", B)] if select else [])
            + [("nerf_amd_param_gradients_finish_bucket", "main", P)])


def masked_guided(Pc, C, select):
    return ([(FETCH, "main", None),
             ("nerf_amd_sample_pdf_volume_masked", "main", Pc),              # places and marks: no nerf_amd_occupancy_mark
             ("nerf_amd_occupancy_points_capped", "main", C),
             ("nerf_amd_mlp_forward_train_points", "main", C),
             ("nerf_amd_volume_render_masked_mse_backward", "main", C),
             ("nerf_amd_mlp_backward", "main", C),
             ("nerf_amd_encode_points_bf16", "side", C),
             ("nerf_amd_mse_loss", "side", 3 * B),
             ("nerf_amd_param_gradients_begin", "side", C)]
            + ([(SELECT, "side", B)] if select else [])
            + [("nerf_amd_param_gradients_finish_bucket", "main", C)])


# The two steppers with a per-image table fetch a second set of scalars: the cut in front of every fetch leaves the step's
# own fetch as a piece of its own, and the rest starts at the table's.
def camera(P):
    return [(FETCH, "main", None),                                          # the camera Adam's scalars
            ("nerf_amd_camera_rays", "main", B),                            # the step's rays from the ids and the poses
            ("nerf_amd_mlp_forward_train", "main", P),
            ("nerf_amd_volume_render_mse_backward", "main", P),
            ("nerf_amd_mlp_backward", "main", P),
            ("nerf_amd_input_gradients", "main", P),                        # behind the dX chain, on the main branch
            ("nerf_amd_camera_rays_backward", "main", B),
            ("nerf_amd_sample_encode_bf16", "side", P),
            ("nerf_amd_mse_loss", "side", 3 * B),
            ("nerf_amd_param_gradients_begin", "side", P),
            (SELECT, "side", B),
            ("nerf_amd_param_gradients_finish_bucket", "main", P)]


def appearance(P):
    return [(FETCH, "main", None),                                          # the appearance Adam's scalars
            ("nerf_amd_appearance_gather", "main", B),                      # one row of theta per ray
            ("nerf_amd_mlp_forward_train", "main", P),
            ("nerf_amd_volume_render_mse_backward_affine", "main", P),
            ("nerf_amd_mlp_backward", "main", P),
            ("nerf_amd_appearance_reduce", "main", B),                      # behind the dX chain, on the main branch
            ("nerf_amd_sample_encode_bf16", "side", P),
            ("nerf_amd_mse_loss", "side", 3 * B),
            ("nerf_amd_param_gradients_begin", "side", P),
            (SELECT, "side", B),
            ("nerf_amd_param_gradients_finish_bucket", "main", P)]


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


def run_case(monkeypatch, dev, synthetic, n_nets, build, step, want, warmup_tail, select, table_adam=None):
    """build(nets, opt) -> stepper under the recorder; step(stepper) runs one iteration.  ``want`` is the forward / backward
    sequence, ``warmup_tail`` what the warm-up enqueues behind its copy of it (the dense stepper warms the head-gradient
    launch of its two-bucket form up too).  ``table_adam`` = the element count of a per-image table with an Adam of its own:
    the step's own fetch is then a piece in front of ``want`` (which starts at the table's fetch), and the table's Adam a
    piece behind the update."""
    from nerf_simple_amd import _lib
    from nerf_simple_amd.optim import FusedAdam
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    nets = make_nets(dev, synthetic, n_nets)
    opt = FusedAdam(nets if n_nets > 1 else nets[0], lr=0.0)
    rec.take()
    stepper = build(nets, opt)
    got = sequences(rec.take())
    lead = [[(FETCH, "main", None)]] if table_adam else []
    upd = [update(opt.flat.numel(), n_nets)] + ([[(ADAM, "main", table_adam)]] if table_adam else [])
    # one process, no exchange: the warm-up, graph A, graph B, then the whole iteration as one graph
    assert stepper.graph_ab is not None and stepper.graph_a2 is None
    parts = (("warm-up", lead + [want + warmup_tail]), ("graph A", lead + [want]), ("graph B", upd),
             ("graph AB: forward / backward", lead + [want]), ("graph AB: update", upd))
    names = [name for name, pieces in parts for _ in pieces]
    wanted = [piece for _, pieces in parts for piece in pieces]
    assert len(got) == len(wanted), [p[0][0] for p in got]
    for name, g, w in zip(names, got, wanted):
        assert g == w, (name, [x for x in zip(g, w) if x[0] != x[1]][:3], len(g), len(w))
    n, a, ab = len(lead), len(lead) + 1, 2 * (len(lead) + 1) + len(upd)
    assert got[a:2 * a] == got[ab:ab + a] and got[n][:len(want)] == got[a + n]     # the warm-up and the captures are one sequence
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


@pytest.mark.parametrize("variant", JITTER)
def test_dense_step_background_and_noise(monkeypatch, dev, synthetic, inputs, variant):
    from nerf_simple_amd.training import GraphedTrainStep
    P, select = B * N, variant == JITTER[1]
    kw = dict(background=torch.tensor([1.0, 0.5, 0.25]), sigma_noise=0.5, noise_seed=5, **jitter_kw(variant, inputs))
    want = dense_controls(P, select)
    run_case(monkeypatch, dev, synthetic, 1, lambda nets, opt: GraphedTrainStep(nets[0], opt, B, N, **kw),
             lambda s: s.step() if select else s.step(inputs["rays"], inputs["gt"], u=inputs["u"]), want,
             [(want[-1][0], "main", P)], select)


@pytest.mark.parametrize("variant", JITTER)
def test_dense_step_distortion(monkeypatch, dev, synthetic, inputs, variant):
    from nerf_simple_amd.training import GraphedTrainStep
    P, select = B * N, variant == JITTER[1]
    want = dense_distortion(P, select)
    run_case(monkeypatch, dev, synthetic, 1,
             lambda nets, opt: GraphedTrainStep(nets[0], opt, B, N, distortion=0.01, **jitter_kw(variant, inputs)),
             lambda s: s.step() if select else s.step(inputs["rays"], inputs["gt"], u=inputs["u"]), want,
             [(want[-1][0], "main", P)], select)


@pytest.mark.parametrize("variant", JITTER)
def test_guided_step(monkeypatch, dev, synthetic, inputs, variant):
    from nerf_simple_amd.training import GraphedGuidedTrainStep
    from nerf_simple_amd.utils.proposal import ProposalVolume
    select = variant == JITTER[1]
    prop = ProposalVolume(17, BOUNDS, device=dev)
    run_case(monkeypatch, dev, synthetic, 1,
             lambda nets, opt: GraphedGuidedTrainStep(nets[0], opt, B, NC, NF, prop, **jitter_kw(variant, inputs)),
             lambda s: s.step() if select else s.step(inputs["rays"], inputs["gt"], u_c=inputs["u_c"], u_f=inputs["u_f"]),
             guided(B * NC, B * (NC + NF), select), [], select)


@pytest.mark.parametrize("variant", JITTER)
def test_masked_guided_step(monkeypatch, dev, synthetic, inputs, variant):
    from nerf_simple_amd.training import GraphedMaskedGuidedTrainStep
    from nerf_simple_amd.utils.proposal import ProposalVolume
    select = variant == JITTER[1]
    C = math.ceil(0.5 * B * (NC + NF))
    prop = ProposalVolume(17, BOUNDS, device=dev)
    s = run_case(monkeypatch, dev, synthetic, 1,
                 lambda nets, opt: GraphedMaskedGuidedTrainStep(nets[0], opt, B, NC, NF, prop, inputs["occ"], 0.5,
                                                                **jitter_kw(variant, inputs)),
                 lambda s: s.step() if select else s.step(inputs["rays"], inputs["gt"], u_c=inputs["u_c"], u_f=inputs["u_f"]),
                 masked_guided(B * NC, C, select), [], select)
    assert s.capacity == C


TABLE_M, TABLE_SIDE = 3, 5          # the smallest table that holds a batch: 3 images of 5 x 5 = 75 rows for B = 37


@pytest.fixture(scope="module")
def image_table(dev, oracle, synthetic):
    """A ray generator over TABLE_M images of TABLE_SIDE x TABLE_SIDE pixels, built image by image from their poses"""
    from nerf_simple_amd.utils.dataload import RayGenerator
    cam = [TABLE_SIDE, TABLE_SIDE, synthetic.focal_from_fov(TABLE_SIDE)]
    colours = torch.rand(TABLE_M, TABLE_SIDE, TABLE_SIDE, 3, generator=torch.Generator().manual_seed(5)).numpy()
    poses = [np.asarray(oracle.spherical_to_pose(4, -30 - 5 * m, 90 * m), dtype=np.float32) for m in range(TABLE_M)]
    return RayGenerator.from_samples({"train": [{"img": im, "transform": p} for im, p in zip(colours, poses)]}, cam, dev)


def test_camera_step(monkeypatch, dev, synthetic, image_table):
    from nerf_simple_amd.training import GraphedCameraTrainStep
    from nerf_simple_amd.utils.cameras import CameraRefinement
    cams = CameraRefinement.from_ray_generator(image_table)
    assert cams.n_rays == TABLE_M * TABLE_SIDE * TABLE_SIDE
    s = run_case(monkeypatch, dev, synthetic, 1,
                 lambda nets, opt: GraphedCameraTrainStep(nets[0], opt, B, N, cams, rays_from=image_table, device_rng=True, seed=11),
                 lambda s: s.step(), camera(B * N), [], True, table_adam=TABLE_M * 6)
    assert s.camera_steps == 1


def test_appearance_step(monkeypatch, dev, synthetic, image_table):
    from nerf_simple_amd.training import GraphedAppearanceTrainStep
    from nerf_simple_amd.utils.appearance import AppearanceCorrection
    app = AppearanceCorrection.from_ray_generator(image_table)
    assert (app.M, app.HW) == (TABLE_M, TABLE_SIDE * TABLE_SIDE)
    want = appearance(B * N)
    s = run_case(monkeypatch, dev, synthetic, 1,
                 lambda nets, opt: GraphedAppearanceTrainStep(nets[0], opt, B, N, app, rays_from=image_table, device_rng=True, seed=11),
                 lambda s: s.step(), want, [(want[-1][0], "main", B * N)], True, table_adam=TABLE_M * 6)
    assert s.appearance_steps == 1
