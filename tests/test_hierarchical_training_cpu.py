"""CPU-side checks of the hierarchical (coarse + fine) training step: the C-ABI argument errors of its coarse-head entry
point nerf_amd_volume_render_mse_backward_pdf, and the pair's checks in training.train_step_hierarchical, which run before
anything is drawn or launched (torch's CPU generator is left untouched).  No GPU needed."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_coarse_head_is_declared_and_exported(lib):
    from nerf_simple_amd import _lib
    assert "nerf_amd_volume_render_mse_backward_pdf" in _lib.EXPORTS
    assert "nerf_amd_volume_render_mse_backward_pdf" in open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    assert hasattr(lib, "nerf_amd_volume_render_mse_backward_pdf")


def test_coarse_head_argument_errors(lib):
    """EINVAL / EUNSUP before anything is launched (the dummy pointers are never dereferenced)."""
    EINVAL, EUNSUP = -1, -2
    DEVICE_RNG, SEED_IN_MEMORY, TS_GIVEN = 2, 4, 1
    null = None
    one = ctypes.c_void_p(16)
    f = lib.nerf_amd_volume_render_mse_backward_pdf

    def call(raw=one, ts=one, rays=one, target=one, u=one, flags=0, rgb=one, d_raw=one, ts_out=one, B=4, Nc=64, Nf=128):
        return f(raw, ts, rays, target, u, flags, 0, 0, rgb, d_raw, ts_out, B, Nc, Nf, null)

    # sizes
    assert call(B=-1) == EINVAL
    assert call(Nc=0) == EINVAL
    assert call(Nf=-1) == EINVAL
    # nerf_amd_sample_pdf's limits: 3 <= Nc <= 256, Nc + Nf <= 512
    assert call(Nc=2) == EUNSUP
    assert call(Nc=257, Nf=0) == EUNSUP
    assert call(Nc=256, Nf=257) == EUNSUP
    assert call(Nc=3, Nf=510) == EUNSUP
    # pointers (rgb alone may be NULL)
    for k in ("raw", "ts", "rays", "target", "d_raw", "ts_out"):
        assert call(**{k: null}) == EINVAL, k
    # jitter: explicit u needs u; unknown flags; seed in memory needs the counter RNG and an 8-byte aligned address
    assert call(u=null) == EINVAL
    assert call(flags=TS_GIVEN) == EINVAL
    assert call(flags=8) == EINVAL
    assert call(flags=SEED_IN_MEMORY) == EINVAL
    assert call(flags=DEVICE_RNG | SEED_IN_MEMORY, u=null) == EINVAL
    assert call(flags=DEVICE_RNG | SEED_IN_MEMORY, u=ctypes.c_void_p(20)) == EINVAL
    # B == 0 launches nothing and succeeds
    assert call(B=0) == 0


def test_pair_checks_before_any_draw():
    """The same module twice, mismatched precisions, Nc < 3 or Nc + Nf > 512 raise before torch's CPU generator moves."""
    from nerf_simple_amd.utils.nets import Nerf
    from nerf_simple_amd.training import train_step_hierarchical, GraphedHierarchicalTrainStep
    net_c, net_f = Nerf(precision="bf16"), Nerf(precision="bf16")
    rays, gt = torch.zeros(8, 6), torch.zeros(8, 3)
    opt = torch.optim.SGD(list(net_c.parameters()) + list(net_f.parameters()), lr=0.0)
    cases = [
        dict(net_c=net_c, net_f=net_c),                                          # the same module twice
        dict(net_c=net_c, net_f=Nerf(precision="fp32")),                         # two precisions
        dict(net_c=net_c, net_f=net_f, Nc=2),
        dict(net_c=net_c, net_f=net_f, Nc=257, Nf=0),
        dict(net_c=net_c, net_f=net_f, Nc=64, Nf=449),
        dict(net_c=net_c, net_f=net_f, Nf=-1),
    ]
    state = torch.get_rng_state()                  # (building the modules above draws their initial weights)
    for kw in cases:
        a = dict(Nc=64, Nf=128)
        a.update({k: v for k, v in kw.items() if k in ("Nc", "Nf")})
        with pytest.raises(ValueError):
            train_step_hierarchical(kw["net_c"], kw["net_f"], opt, rays, gt, a["Nc"], a["Nf"])
        with pytest.raises(ValueError):
            GraphedHierarchicalTrainStep(kw["net_c"], kw["net_f"], opt, 8, a["Nc"], a["Nf"])
    assert torch.equal(torch.get_rng_state(), state)


def test_train_step_hierarchical_rejects_a_foreign_optimizer():
    from nerf_simple_amd.utils.nets import Nerf
    from nerf_simple_amd.training import train_step_hierarchical
    net_c, net_f = Nerf(precision="bf16"), Nerf(precision="bf16")
    only_c = torch.optim.SGD(net_c.parameters(), lr=0.0)
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="optimizer"):
        train_step_hierarchical(net_c, net_f, only_c, torch.zeros(8, 6), torch.zeros(8, 3))
    assert torch.equal(torch.get_rng_state(), state)
