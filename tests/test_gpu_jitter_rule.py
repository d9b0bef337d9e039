"""DESIGN.md section 31 on the device: for every row of its table the entry point's DEFAULT jitter is the ``torch.rand(B, n)``
calls the table names, in that order -- the same call with those draws made by the caller and handed in gives the same
bits and leaves torch's CPU generator in the same state.  The rows (entry point, draws, call) are tools/entry_bytes.py's,
which prints their hashes; 37 rays, N = 5, Nc = 5, Nf = 3, bf16, structured weights, a ball grid and a proposal volume at 16.

No older test asserts one of these rows exactly (bits AND generator state, default against handed-in draws), so none is left
out; what the older ones pin is next to it: the draw itself against the reference's stream and the image drivers'
``ReferenceJitter`` (tests/test_gpu_parity.py), "a refused call draws nothing" per entry point (the files of each feature).
"""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("entry_bytes", os.path.join(ROOT, "tools", "entry_bytes.py"))
entry_bytes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(entry_bytes)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eb():
    return entry_bytes


@pytest.fixture(scope="module")
def scene():
    return entry_bytes.scene(torch.device("cuda:0"))


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), i
        if x is not None:
            assert x.shape == y.shape and x.dtype == y.dtype, i
            # bit for bit (NaN disparities included): compare the bytes, not the values
            assert torch.equal(x.detach().reshape(-1).view(torch.uint8), y.detach().reshape(-1).view(torch.uint8)), i


def _close_gradients(a, b, P):
    """The flat gradient of a train step is the one output that is not reproducible bit for bit, whatever the jitter: the dW
    products combine their split-K partial sums with float atomics (csrc/dw_gemm.hip; training.py's docstring), in an order
    that differs from run to run.  The same jitter gives the same addends, so two runs differ by a reordering of at most P
    fp32 addends per element (P: the sample rows of the largest pass here, 37 x 8): at most 2 (P - 1) 2^-24 sum|addend|
    (Higham, Accuracy and Stability, section 4.2), and sum|addend| is taken as at most P times the largest gradient magnitude.
    Another jitter moves the gradient by its own size.  The loss and the positions, compared bit for bit beside it, see
    every sample."""
    scale = float(torch.maximum(a.abs().max(), b.abs().max()))
    worst = float((a - b).abs().max())
    bound = 2.0 * (P - 1) * 2.0 ** -24 * P * scale
    print(f"gradients: max|difference| = {worst:.3e}, max|gradient| = {scale:.3e}, bound = {bound:.3e}")
    assert torch.isfinite(a).all() and scale > 0 and worst <= bound


@pytest.mark.parametrize("row", [pytest.param(r, id=r[0].replace(" ", "-")) for r in entry_bytes.ROWS])
def test_default_jitter_is_the_tables_draws(eb, scene, row):
    drawn, state_drawn = eb.run(scene, row, "default")
    given, state_given = eb.run(scene, row, "explicit")
    assert any(t is not None and t.numel() for t in drawn)
    if eb.has_grads(row):
        _close_gradients(drawn[-1], given[-1], eb.B * (eb.NC + eb.NF))
        drawn, given = drawn[:-1], given[:-1]
    _same(drawn, given)
    assert torch.equal(state_drawn, state_given)
    # and the draws were taken: the generator is not where the seed put it
    torch.manual_seed(eb.SEED)
    assert not torch.equal(state_drawn, torch.get_rng_state())


def _row(eb, name):
    return next(r for r in eb.ROWS if r[0] == name)


@pytest.mark.parametrize("masked", (False, True), ids=("dense", "occupancy"))
def test_render_hierarchical_a_given_u_c_wins_over_device_rng(eb, scene, masked):
    """The pair rule: with u_c AND device_rng=True the coarse pass runs on u_c (its 5-tuple is that of u_c alone, which
    draws u_f from the CPU generator); only the fine samples come from the counter RNG."""
    row = _row(eb, "render_hierarchical" + (" occupancy=" if masked else ""))
    torch.manual_seed(99)
    u_c = torch.rand(eb.B, eb.NC).to(scene.dev)
    both, state_both = eb.run(scene, row, "device_rng", u_c=u_c)
    alone, _ = eb.run(scene, row, "default", u_c=u_c)
    _same(both[5:10], alone[5:10])
    torch.manual_seed(eb.SEED)
    assert torch.equal(state_both, torch.get_rng_state())          # nothing was drawn: u_c given, u_f from the counter RNG


@pytest.mark.parametrize("masked", (False, True), ids=("dense", "occupancy"))
def test_render_hierarchical_view_device_rng_drops_given_uniforms(eb, scene, masked):
    """This entry point's own rule: with device_rng=True a given u_c is not looked at."""
    row = _row(eb, "render_hierarchical_view" + (" occupancy=" if masked else ""))
    torch.manual_seed(99)
    u_c = torch.rand(eb.B, eb.NC).to(scene.dev)
    both, _ = eb.run(scene, row, "device_rng", u_c=u_c)
    alone, _ = eb.run(scene, row, "device_rng")
    _same(both, alone)
    with_u_c, _ = eb.run(scene, row, "default", u_c=u_c)
    assert not torch.equal(with_u_c[0], alone[0])                   # without device_rng the same u_c does matter


def test_proposal_refuses_u_c_with_device_rng(eb, scene):
    """ProposalVolume.check's own rule, before any draw."""
    torch.manual_seed(eb.SEED)
    before = torch.get_rng_state()
    u_c = torch.zeros(eb.B, eb.NC, device=scene.dev)
    with pytest.raises(ValueError, match="cannot be combined with u_c"):
        scene.prop.sample(scene.rays, eb.NC, eb.NF, u_c=u_c, device_rng=True)
    assert torch.equal(before, torch.get_rng_state())
