#!/usr/bin/env python3
"""The bytes the eager entry points produce, one line per (entry point, jitter mode): the sha256 of every output tensor and
of torch's CPU generator state behind the call.  Two trees whose lines are equal compute the same thing and advance the
generator the same way; that is how a change to the Python boundary shows that it moved nothing.

    python tools/entry_bytes.py > bytes.txt          # in each tree, a fresh process each; then diff the two files

``ROWS`` is also the table tests/test_gpu_jitter_rule.py walks: per entry point the call and the ``torch.rand(B, n)``
draws section 31 says its default jitter makes, in order.  Shapes: 37 rays (no multiple of the wave), N = 5, Nc = 5, Nf = 3,
bf16, structured synthetic weights, a ball occupancy grid and a proposal volume at resolution 16.  Reads nothing outside
the repository.

The train rows end in the flat gradient, which is NOT hashed: the dW products combine their split-K partial sums with float
atomics (csrc/dw_gemm.hip), so its last bits differ between two runs of one tree.  Its largest magnitude is printed to three
digits instead; the loss, which every sample feeds, is hashed like everything else.

``CONTROL_ROWS`` are the same entry points with the training controls on; ``main`` prints them behind
``ROWS``.
"""
import hashlib
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_simple_amd import training as T                                              # noqa: E402
from nerf_simple_amd.utils import rendering as R, synthetic                            # noqa: E402
from nerf_simple_amd.utils.mesh import DEFAULT_BOUNDS                                   # noqa: E402
from nerf_simple_amd.utils.nets import Nerf                                             # noqa: E402
from nerf_simple_amd.utils.occupancy import EarlyTermination, OccupancyGrid             # noqa: E402
from nerf_simple_amd.utils.proposal import ProposalVolume                               # noqa: E402
from nerf_simple_amd.utils.xyz import spherical_to_pose                                 # noqa: E402

B, N, NC, NF, RES, SEED = 37, 5, 5, 3, 16, 1234


def scene(dev):
    """Everything the rows share; built once, never written to (the train rows step with lr = 0)."""
    def net_on(seed):
        net = Nerf(precision="bf16").to(dev)
        net.load_state_dict(synthetic.synthetic_state_dict(seed, "structured"))
        return net
    s = SimpleNamespace(dev=dev, net=net_on(0), net_c=net_on(1), net_f=net_on(2))
    s.pose, s.cam = spherical_to_pose(4, -30, 0), (7, 7, synthetic.focal_from_fov(7))
    s.rays = R.generate_rays(s.pose, s.cam, dev, 0, B)
    s.gt = torch.rand(B, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    c = (torch.arange(RES - 1, dtype=torch.float64, device=dev) + 0.5) * (3.0 / (RES - 1)) - 1.5
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    s.occ = OccupancyGrid.from_mask(X * X + Y * Y + Z * Z <= 1.2 * 1.2, DEFAULT_BOUNDS, outside="empty")
    s.prop = ProposalVolume(RES, DEFAULT_BOUNDS, device=dev).update(s.net)
    # sample_pdf's inputs: rising positions and positive weights, different on every ray
    i = torch.arange(B * NC, dtype=torch.float32, device=dev).view(B, NC)
    s.ts_c = torch.linspace(2.2, 5.8, NC, device=dev).expand(B, NC) + 0.01 * i[:, :1] / NC
    s.w_c = ((i * 7) % 11 + 1) / 12
    return s


def _sgd(*nets):
    return torch.optim.SGD([p for n in nets for p in n.parameters()], lr=0.0)


def _grads(*nets):
    return torch.cat([p.grad.reshape(-1) for n in nets for p in n.parameters()])


def _flat(out):
    """Nested tuples of tensors (and MarkResults) -> one flat tuple of tensors / None."""
    if out is None or torch.is_tensor(out):
        return (out,)
    if hasattr(out, "offsets"):
        return (out.mask, out.offsets)
    return tuple(t for o in out for t in _flat(o))


def _train(s, occ, **jit):
    loss = T.train_step(s.net, _sgd(s.net), s.rays, s.gt, N, occupancy=occ, **jit)
    return loss, _grads(s.net)


def _train_pair(s, occ, **jit):
    loss = T.train_step_hierarchical(s.net_c, s.net_f, _sgd(s.net_c, s.net_f), s.rays, s.gt, NC, NF, occupancy=occ, **jit)
    return loss, loss.losses[0], loss.losses[1], loss.ts_f, _grads(s.net_c, s.net_f)


def _train_guided(s, occ, **jit):
    loss = T.train_step_guided(s.net, _sgd(s.net), s.rays, s.gt, NC, NF, s.prop, occupancy=occ, **jit)
    return loss, loss.ts, _grads(s.net)


ONE, FINE, PAIR = (("u", N),), (("u", NF),), (("u_c", NC), ("u_f", NF))
TERM = dict(eps=1e-3, slab=16)
# (name, grad enabled, the default jitter's torch.rand(B, n) draws as (keyword, n) in order, call(scene, **jitter keywords))
ROWS = (
    ("render_nerf", False, ONE, lambda s, **j: R.render_nerf(s.rays, s.net, N, **j)),
    ("render_nerf occupancy=", False, ONE, lambda s, **j: R.render_nerf(s.rays, s.net, N, occupancy=s.occ, **j)),
    ("render_nerf terminate=", False, ONE,
     lambda s, **j: R.render_nerf(s.rays, s.net, N, terminate=EarlyTermination(**TERM), **j)),
    ("render_view", False, ONE, lambda s, **j: R.render_view(s.net, s.pose, s.cam, N=N, n_rays=B, **j)),
    ("render_view background=", False, ONE,
     lambda s, **j: R.render_view(s.net, s.pose, s.cam, N=N, n_rays=B, background=(0.2, 0.4, 0.6), **j)),
    ("render_view occupancy=", False, ONE, lambda s, **j: R.render_view(s.net, s.pose, s.cam, N=N, n_rays=B, occupancy=s.occ, **j)),
    ("sample_pdf", False, FINE, lambda s, **j: R.sample_pdf(s.ts_c, s.w_c, NF, **j)),
    ("render_hierarchical", False, PAIR, lambda s, **j: R.render_hierarchical(s.rays, s.net_c, s.net_f, NC, NF, **j)),
    ("render_hierarchical occupancy=", False, PAIR,
     lambda s, **j: R.render_hierarchical(s.rays, s.net_c, s.net_f, NC, NF, occupancy=s.occ, **j)),
    ("render_hierarchical_view", False, PAIR,
     lambda s, **j: R.render_hierarchical_view(s.net_c, s.net_f, s.pose, s.cam, NC, NF, n_rays=B, **j)),
    ("render_hierarchical_view occupancy=", False, PAIR,
     lambda s, **j: R.render_hierarchical_view(s.net_c, s.net_f, s.pose, s.cam, NC, NF, n_rays=B, occupancy=s.occ, **j)),
    ("ProposalVolume.sample", False, PAIR, lambda s, **j: s.prop.sample(s.rays, NC, NF, return_weights=True, **j)),
    ("ProposalVolume.sample occupancy=", False, PAIR,
     lambda s, **j: s.prop.sample(s.rays, NC, NF, return_weights=True, occupancy=s.occ, return_mark=True, **j)),
    ("render_guided", False, PAIR, lambda s, **j: R.render_guided(s.rays, s.net, NC, NF, s.prop, **j)),
    ("render_guided occupancy=", False, PAIR, lambda s, **j: R.render_guided(s.rays, s.net, NC, NF, s.prop, occupancy=s.occ, **j)),
    ("render_nerf_masked", True, ONE, lambda s, **j: T.render_nerf_masked(s.rays, s.net, N, s.occ, **j)),
    ("train_step", True, ONE, lambda s, **j: _train(s, None, **j)),
    ("train_step occupancy=", True, ONE, lambda s, **j: _train(s, s.occ, **j)),
    ("train_step_hierarchical", True, PAIR, lambda s, **j: _train_pair(s, None, **j)),
    ("train_step_hierarchical occupancy=", True, PAIR, lambda s, **j: _train_pair(s, s.occ, **j)),
    ("train_step_guided", True, PAIR, lambda s, **j: _train_guided(s, None, **j)),
    ("train_step_guided occupancy=", True, PAIR, lambda s, **j: _train_guided(s, s.occ, **j)),
)

# The same entry points with the training controls on: one fixed bundle, each row with the pieces its
# entry point accepts.  ``train_step`` appears with the four flat keywords and with ``controls=``: the two rows print the same
# digests.
BG, LAM = (0.2, 0.4, 0.6), 0.01
C_BG = T.Controls(background=BG)
C_NOISE = T.Controls(background=BG, sigma_noise=0.5, noise_seed=11)
C_ALL = C_NOISE.replace(distortion=LAM)


def _per_ray(s):
    """One colour per ray [B,3], different on every ray."""
    return T.Controls(background=torch.rand(B, 3, generator=torch.Generator().manual_seed(2)).to(s.dev))


CONTROL_ROWS = (
    ("render_nerf background=", False, ONE, lambda s, **j: R.render_nerf(s.rays, s.net, N, background=BG, **j)),
    ("render_nerf controls= occupancy=", False, ONE,
     lambda s, **j: R.render_nerf(s.rays, s.net, N, occupancy=s.occ, controls=_per_ray(s), **j)),
    ("render_view controls= occupancy=", False, ONE,
     lambda s, **j: R.render_view(s.net, s.pose, s.cam, N=N, n_rays=B, occupancy=s.occ, controls=C_BG, **j)),
    ("render_hierarchical controls=", False, PAIR,
     lambda s, **j: R.render_hierarchical(s.rays, s.net_c, s.net_f, NC, NF, controls=C_BG, **j)),
    ("render_hierarchical controls= occupancy=", False, PAIR,
     lambda s, **j: R.render_hierarchical(s.rays, s.net_c, s.net_f, NC, NF, occupancy=s.occ, controls=C_BG, **j)),
    ("render_hierarchical_view controls=", False, PAIR,
     lambda s, **j: R.render_hierarchical_view(s.net_c, s.net_f, s.pose, s.cam, NC, NF, n_rays=B, controls=C_BG, **j)),
    ("render_hierarchical_view controls= occupancy=", False, PAIR,
     lambda s, **j: R.render_hierarchical_view(s.net_c, s.net_f, s.pose, s.cam, NC, NF, n_rays=B, occupancy=s.occ, controls=C_BG,
                                               **j)),
    ("render_nerf_masked controls=", True, ONE, lambda s, **j: T.render_nerf_masked(s.rays, s.net, N, s.occ, controls=C_NOISE, **j)),
    ("train_step flat keywords", True, ONE,
     lambda s, **j: _train(s, None, background=BG, sigma_noise=0.5, noise_seed=11, distortion=LAM, **j)),
    ("train_step controls=", True, ONE, lambda s, **j: _train(s, None, controls=C_ALL, **j)),
    ("train_step occupancy= controls=", True, ONE, lambda s, **j: _train(s, s.occ, controls=C_ALL, **j)),
    ("train_step_hierarchical controls=", True, PAIR, lambda s, **j: _train_pair(s, None, controls=C_NOISE, **j)),
    ("train_step_hierarchical occupancy= controls=", True, PAIR, lambda s, **j: _train_pair(s, s.occ, controls=C_NOISE, **j)),
    ("train_step_guided distortion=", True, PAIR, lambda s, **j: _train_guided(s, None, distortion=LAM, **j)),
    ("train_step_guided occupancy= controls=", True, PAIR, lambda s, **j: _train_guided(s, s.occ, controls=C_ALL, **j)),
)


def run(s, row, mode, **extra):
    """One call of ``row`` from the fixed seed -> (flat outputs, generator state behind it).  mode 'default': the entry
    point draws; 'explicit': the caller makes the row's torch.rand draws and hands them in; 'device_rng': the counter RNG."""
    _, grad, draws, call = row
    torch.manual_seed(SEED)
    jit = dict(extra)
    if mode == "explicit":
        jit.update({kw: torch.rand(B, n).to(s.dev) for kw, n in draws})
    elif mode == "device_rng":
        jit.update(device_rng=True, seed=7)
    with torch.set_grad_enabled(grad):
        out = _flat(call(s, **jit))
    torch.cuda.synchronize(s.dev)
    return out, torch.get_rng_state()


def has_grads(row):
    """The row's last output is the flat gradient of a train step (reproducible to reassociation only)."""
    return row[0].startswith("train_step")


def digest(t):
    return "-" * 12 if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:12]


def main():
    assert torch.cuda.is_available(), "the entry points run on the GPU; there is nothing to hash without one"
    s = scene(torch.device("cuda:0"))
    for row in ROWS + CONTROL_ROWS:
        for mode in ("default", "explicit", "device_rng"):
            out, state = run(s, row, mode)
            tail = ""
            if has_grads(row):
                out, tail = out[:-1], f" max|grad|={float(out[-1].abs().max()):.2e}"
            print(f"{row[0]:38s} {mode:10s} {' '.join(digest(t) for t in out)}{tail} rng={digest(state)}", flush=True)


if __name__ == "__main__":
    main()
