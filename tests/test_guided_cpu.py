"""Grid-guided fine sampling without a GPU (include/nerf_amd.h, "grid-guided fine sampling"): the new
entry point is exported, bound and declared with one prototype; its argument rules are pinned call by call
(tests/golden/abi_refusals_guided.json, the format of abi_refusals.json: every call is refused or is an empty problem, so
nothing is launched and no pointer is dereferenced); the numpy model (tests/guided_model.py) has the properties the
definition states; and a refused Python call leaves torch's CPU generator untouched.

`python tests/test_guided_cpu.py` re-records the return values of the fixture from the library in the tree."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import guided_model as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_refusals_guided.json")
NEW = "nerf_amd_sample_pdf_volume"
FAKE = 0x1000
EINVAL, EUNSUP = -1, -2
BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))

with open(FIXTURE) as _f:
    CASES = json.load(_f)


def call(lib, case):
    return getattr(lib, case["fn"])(*[FAKE if a == "P" else a for a in case["args"]])


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- the library ---------------------------------------------------------------------------------------------------------
def test_symbol_exported_bound_and_declared_once(lib):
    from nerf_simple_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, NEW) and NEW in _lib.EXPORTS and len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    f = getattr(lib, NEW)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert f.restype is i32
    assert list(f.argtypes) == [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, i64, vp, i64, i64, i64, vp, vp, vp, vp, vp, vp,
                                i64, i32, i32, vp]
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.findall(r"\bint\s+" + NEW + r"\s*\(([^)]*)\)\s*;", code)
    assert len(m) == 1
    params = [" ".join(p.split()) for p in m[0].split(",")]
    assert params == ["const float* rays", "const float* u", "const float* tbins", "uint32_t flags", "uint64_t seed",
                      "int64_t ray_id0", "const float* sigma_volume", "int64_t nx", "int64_t ny", "int64_t nz",
                      "const float* h_lo", "const float* h_inv_step", "const float* u_f", "float* ts_out", "float* sigma_c",
                      "float* w_c", "int64_t B", "int Nc", "int Nf", "void* stream"]
    assert lib.nerf_amd_abi_version() == 5 and "#define NERF_AMD_ABI_VERSION 5" in header


def test_fixture_covers_every_limit():
    """Both sides of each limit, the axis rule and the order of EINVAL against EUNSUP are in the fixture."""
    from nerf_simple_amd import _lib
    nc, total, rays, axes, two = set(), set(), set(), set(), 0
    for c in CASES:
        assert c["fn"] == NEW and len(c["args"]) == len(_lib._SIGNATURES[NEW][1]), c
        a = c["args"]
        nc.add(a[17]); total.add(a[17] + a[18]); rays.add(a[16]); axes.update(a[7:10])
        two += c["note"].startswith("two rules:")
    assert {2, 3, 256, 257} <= nc and {512, 513} <= total and {2 ** 32, 2 ** 32 + 1} <= rays and {1, 2} <= axes
    assert two >= 2
    by = {c["note"]: c["expect"] for c in CASES}
    assert len(by) == len(CASES)                       # every note names one case
    assert {c["expect"] for c in CASES} == {0, EINVAL, EUNSUP}


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"{i}-{CASES[i]['note'][:40]}")
def test_abi_refusal(lib, i):
    case = CASES[i]
    assert call(lib, case) == case["expect"], (case["note"], case["args"])


def test_the_two_sides_of_a_limit_differ(lib):
    """On the passing side of a size limit the call gets as far as the missing ts_out (EINVAL); beyond it, EUNSUP."""
    def f(B=4, Nc=64, Nf=128, axis=4, ts_out=None):
        return lib.nerf_amd_sample_pdf_volume(FAKE, FAKE, FAKE, 0, 0, 0, FAKE, axis, 4, 4, FAKE, FAKE, FAKE, ts_out, None, None,
                                              B, Nc, Nf, None)
    assert f() == EINVAL
    for ok, bad in ((dict(Nc=3, Nf=1), dict(Nc=2, Nf=1)), (dict(Nc=256, Nf=256), dict(Nc=257, Nf=0)),
                    (dict(Nc=64, Nf=448), dict(Nc=64, Nf=449)), (dict(B=2 ** 32), dict(B=2 ** 32 + 1))):
        assert f(**ok) == EINVAL and f(**bad) == EUNSUP, (ok, bad)
    assert f(B=0, axis=2, ts_out=FAKE) == 0 and f(B=0, axis=1, ts_out=FAKE) == EINVAL
    assert f(B=0, ts_out=None) == 0                    # B = 0 launches nothing and asks for no buffer


# ---- the model -----------------------------------------------------------------------------------------------------------
def _rays(oracle, synthetic, side=6):
    pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, -30, 0))).float()
    return oracle.camera_rays(pose, [side, side, synthetic.focal_from_fov(side)]).contiguous()


def _ts(B, Nc, seed, tn=2, tf=6):
    u = torch.rand(B, Nc, generator=torch.Generator().manual_seed(seed))
    tb = torch.linspace(tn, tf, Nc + 1)
    return (tb[1] - tb[0]) * u + tb[:-1]


def test_model_unknown_volume_gives_the_uniform_placement(oracle, synthetic):
    """All -inf: every weight is exactly 0, so the pdf is the 1e-5 floor's, uniform over the interior bins."""
    rays = _rays(oracle, synthetic)
    B, Nc, Nf, R = rays.shape[0], 16, 24, (5, 4, 3)
    ts_c = _ts(B, Nc, 1)
    u_f = torch.rand(B, Nf, generator=torch.Generator().manual_seed(2))
    lo, _, inv = G.grid_axes(R, BOUNDS)
    ts, sigma_c, w_c = G.guided_sample(oracle, rays, ts_c, np.full(R, -np.inf, np.float32), lo, inv, u_f)
    assert np.all(np.isneginf(sigma_c)) and torch.all(w_c == 0)
    assert torch.equal(ts, oracle.sample_pdf(ts_c, torch.zeros(B, Nc), u_f))
    p = G.pdf(w_c)
    assert torch.all(p == p[:, :1]) and torch.all(torch.isfinite(ts))
    assert torch.all(ts[:, 1:] >= ts[:, :-1])


def test_model_nan_corner_is_skipped_unless_all_eight_are(oracle):
    R = (4, 3, 3)
    lo, step, inv = G.grid_axes(R, BOUNDS)
    rng = np.random.default_rng(0)
    V = (8 * rng.standard_normal(R)).astype(np.float32)
    centre = (lo + step * np.asarray([1.5, 0.5, 1.5], np.float32)).astype(np.float32)[None]       # cell (1, 0, 1)
    inside, c = G.cells(centre, R, lo, inv)
    assert inside[0] and tuple(c[0]) == (1, 0, 1)
    corners = [(1 + (k >> 2), (k >> 1) & 1, 1 + (k & 1)) for k in range(8)]
    want = max(V[i] for i in corners)
    assert G.lookup(centre, V, lo, inv)[0] == want
    order = sorted(corners, key=lambda i: V[i])                      # smallest first: the maximum goes last
    W = V.copy()
    for n, i in enumerate(order[:-1]):
        W[i] = np.nan
        assert G.lookup(centre, W, lo, inv)[0] == want, n            # a NaN corner below the maximum changes nothing
    W[order[-1]] = np.nan
    assert np.isneginf(G.lookup(centre, W, lo, inv)[0])              # all eight: -inf, never NaN
    W = V.copy()
    W[order[-1]] = np.nan                                            # the maximum itself: the next one takes over
    assert G.lookup(centre, W, lo, inv)[0] == V[order[-2]]
    assert not np.any(np.isnan(G.lookup(np.asarray([[np.nan, 0, 0]], np.float32), V, lo, inv)))


def test_model_upper_face_and_beyond_are_outside():
    R = (5, 4, 3)
    lo, step, inv = G.grid_axes(R, BOUNDS)
    V = np.ones(R, np.float32)
    hi = np.asarray(BOUNDS[1], np.float32)
    mid = np.zeros(3, np.float32)
    assert G.lookup(mid[None], V, lo, inv)[0] == 1
    assert G.lookup(lo[None], V, lo, inv)[0] == 1                    # the lower corner is cell 0
    for a in range(3):
        p = mid.copy(); p[a] = hi[a]
        f = np.floor(((p[a] - lo[a]).astype(np.float32) * inv[a]).astype(np.float32))
        assert f == R[a] - 1                                         # the point ON the upper face falls in "cell n - 1"
        assert np.isneginf(G.lookup(p[None], V, lo, inv)[0])
        p[a] = np.nextafter(lo[a], np.float32(-np.inf))
        assert np.isneginf(G.lookup(p[None], V, lo, inv)[0])
        p[a] = np.nan
        assert np.isneginf(G.lookup(p[None], V, lo, inv)[0])


def test_model_hot_slab_takes_the_pdf_mass(oracle, synthetic):
    """One hot slab (sigma = 30 inside, -inf elsewhere): a ray that crosses it puts more than 99 % of the pdf mass into the
    bins of the samples that touch the slab -- the 1e-5 floor's share is at most (Nc - 2) 1e-5 against a weight sum near 1."""
    R = (33, 33, 33)
    lo, step, inv = G.grid_axes(R, BOUNDS)
    V = np.full(R, -np.inf, np.float32)
    V[:, :, 14:19] = 30.0                                            # grid points 14..18 along z: cells 13..18 see a hot corner
    # 36 rays from z = 4 down through the box, aimed at a 6 x 6 lattice on the plane z = 0
    aim = torch.stack(torch.meshgrid(torch.linspace(-1, 1, 6), torch.linspace(-1, 1, 6), indexing="ij"), -1).reshape(-1, 2)
    o = torch.tensor([0.3, -0.2, 4.0]).expand(aim.shape[0], 3)
    d = torch.cat([aim, torch.zeros(aim.shape[0], 1)], 1) - o
    rays = torch.cat([o, d / torch.norm(d, dim=1, keepdim=True)], 1).contiguous()       # unit directions: z = 0 near t = 4
    B, Nc, Nf = rays.shape[0], 64, 128
    ts_c = _ts(B, Nc, 3)
    u_f = torch.rand(B, Nf, generator=torch.Generator().manual_seed(4))
    ts, sigma_c, w_c = G.guided_sample(oracle, rays, ts_c, V, lo, inv, u_f)
    hot = torch.from_numpy(sigma_c == 30.0)
    crossing = hot[:, 1:-1].any(1)
    assert bool(crossing.all())                                       # every ray crosses the slab
    assert set(np.unique(sigma_c)) <= {np.float32(-np.inf), np.float32(30.0)}
    mass = (G.pdf(w_c) * hot[:, 1:-1]).sum(1)
    assert torch.all(mass[crossing] > 0.99), mass[crossing].min()
    assert torch.all(w_c[~hot] == 0)                                  # -inf: alpha = w = 0 exactly
    # and the new samples follow: at least 99 % - 3 sigma of the Nf draws land between the slab's neighbouring mids
    mids = 0.5 * (ts_c[:, 1:] + ts_c[:, :-1])
    for b in torch.nonzero(crossing).flatten().tolist():
        idx = torch.nonzero(hot[b, 1:-1]).flatten() + 1
        t0, t1 = mids[b, idx.min() - 1], mids[b, idx.max()]
        new = int(((ts[b] >= t0) & (ts[b] <= t1)).sum()) - int(((ts_c[b] >= t0) & (ts_c[b] <= t1)).sum())
        assert new >= 0.95 * Nf, (b, new)


# ---- Python refusals -----------------------------------------------------------------------------------------------------
def _host_proposal(R=(5, 4, 3)):
    """A ProposalVolume whose tensor lives on the host: enough for every refusal that comes before a launch."""
    from nerf_simple_amd.utils.proposal import ProposalVolume
    p = ProposalVolume.__new__(ProposalVolume)
    p._init(torch.full(R, float("-inf")), R, BOUNDS)
    return p


def test_python_refusals_leave_the_cpu_generator_untouched():
    from nerf_simple_amd import training
    from nerf_simple_amd.utils import rendering
    from nerf_simple_amd.utils.nets import Nerf
    from nerf_simple_amd.utils.proposal import ProposalVolume
    prop, rays, net, small = _host_proposal(), torch.zeros(4, 6), Nerf(), Nerf(6, 4, 64)      # (initialisation draws)
    torch.manual_seed(1234)
    state = torch.get_rng_state().clone()
    refusals = (
        (RuntimeError, lambda: ProposalVolume(8, device="cpu")),
        (ValueError, lambda: ProposalVolume(1, device="cpu")),
        (ValueError, lambda: prop.sample(rays, 2, 8)),
        (ValueError, lambda: prop.sample(rays, 257, 0)),
        (ValueError, lambda: prop.sample(rays, 64, 449)),
        (ValueError, lambda: prop.sample(rays, 64, -1)),
        (RuntimeError, lambda: prop.sample(rays, 64, 128)),                         # rays on the host: no CPU path
        (RuntimeError, lambda: prop.sample(rays, 64, 128, device_rng=True)),
        (TypeError, lambda: rendering.render_guided(rays, net, 64, 128, object())),
        (RuntimeError, lambda: rendering.render_guided(rays, object(), 64, 128, prop)),
        (RuntimeError, lambda: rendering.render_guided(rays, small, 64, 128, prop)),
        (RuntimeError, lambda: rendering.render_guided(rays, net, 64, 128, prop)),
        (ValueError, lambda: rendering.render_guided(rays, net, 2, 128, prop)),
        (TypeError, lambda: rendering.render_guided_view(net, np.eye(4), [4, 4, 4.0], 64, 128, None)),
        (TypeError, lambda: training.train_step_guided(net, None, rays, rays[:, :3], 64, 128, None)),
        (RuntimeError, lambda: training.train_step_guided(object(), None, rays, rays[:, :3], 64, 128, prop)),
        (ValueError, lambda: training.train_step_guided(net, None, rays, rays[:, :3], 300, 0, prop)),
        (RuntimeError, lambda: training.train_step_guided(net, None, rays, rays[:, :3], 64, 128, prop)),
        (ValueError, lambda: training.GraphedGuidedTrainStep(net, None, 4, 64, 128, prop, storage="e4m3")),
        (ValueError, lambda: training.GraphedGuidedTrainStep(net, None, 4, 64, 128, prop, buckets=2)),
        (TypeError, lambda: training.GraphedGuidedTrainStep(net, None, 4, 64, 128, None)),
        (ValueError, lambda: training.GraphedGuidedTrainStep(net, None, 4, 2, 128, prop)),
    )
    for exc, f in refusals:
        with pytest.raises(exc):
            f()
        assert torch.equal(torch.get_rng_state(), state)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    from nerf_simple_amd import _lib
    for c in CASES:
        c["expect"] = call(_lib.lib(), c)
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in CASES) + "\n]\n")
    print(f"{len(CASES)} cases recorded")
