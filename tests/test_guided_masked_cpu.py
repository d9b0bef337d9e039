"""The masked guided placement without a GPU (include/nerf_amd.h, "masked guided placement"): the new
entry point is exported, bound and declared with one prototype; its argument rules are pinned call by call
(tests/golden/abi_refusals_guided_masked.json, the format of abi_refusals.json: every call is refused or is an empty problem
that writes nothing, so nothing is launched and no pointer is dereferenced); the numpy model (tests/guided_masked_model.py)
has the properties the definition states; the Python surface takes ``occupancy`` by keyword only, and a refused call leaves
torch's CPU generator untouched.

`python tests/test_guided_masked_cpu.py` re-records the return values of the fixture from the library in the tree."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import guided_masked_model as M
import guided_model as G
import occupancy_model as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_refusals_guided_masked.json")
NEW = "nerf_amd_sample_pdf_volume_masked"
FAKE = 0x1000
EINVAL, EUNSUP = -1, -2
BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
PARAMS = ["const float* rays", "const float* u", "const float* tbins", "uint32_t flags", "uint64_t seed", "int64_t ray_id0",
          "const float* sigma_volume", "int64_t vx", "int64_t vy", "int64_t vz", "const float* v_lo", "const float* v_inv_step",
          "const uint32_t* bits", "int64_t gx", "int64_t gy", "int64_t gz", "const float* g_lo", "const float* g_inv_step",
          "const float* u_f", "float* ts_out", "float* sigma_c", "float* w_c", "uint64_t* mask", "int64_t* offsets",
          "int64_t* live", "void* workspace", "int64_t B", "int Nc", "int Nf", "void* stream"]
ARG = {p.split()[-1].lstrip("*"): i for i, p in enumerate(PARAMS)}

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
    kinds = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int64_t": i64, "int": i32}
    assert f.restype is i32
    assert list(f.argtypes) == [vp if "*" in p else kinds[p.split()[0]] for p in PARAMS]
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.findall(r"\bint\s+" + NEW + r"\s*\(([^)]*)\)\s*;", code)
    assert len(m) == 1
    assert [" ".join(p.split()) for p in m[0].split(",")] == PARAMS
    assert lib.nerf_amd_abi_version() == 5 and "#define NERF_AMD_ABI_VERSION 5" in header


def test_fixture_covers_every_limit():
    """Both sides of each size limit and of both axis rules, an unknown flag, every NULL and every misalignment, and the
    doubly-wrong calls that fix the order."""
    from nerf_simple_amd import _lib
    nc, total, rays, vaxes, gaxes, flags, two = set(), set(), set(), set(), set(), set(), 0
    for c in CASES:
        assert c["fn"] == NEW and len(c["args"]) == len(_lib._SIGNATURES[NEW][1]) == len(PARAMS), c
        a = c["args"]
        nc.add(a[ARG["Nc"]]); total.add(a[ARG["Nc"]] + a[ARG["Nf"]]); rays.add(a[ARG["B"]]); flags.add(a[ARG["flags"]])
        vaxes.update(a[ARG["vx"]:ARG["vz"] + 1]); gaxes.update(a[ARG["gx"]:ARG["gz"] + 1])
        two += c["note"].startswith("two rules:")
    assert {2, 3, 256, 257} <= nc and {512, 513} <= total and {2 ** 32, 2 ** 32 + 1} <= rays
    assert {1, 2} <= vaxes and {1, 2} <= gaxes and 128 in flags and two >= 4
    notes = {c["note"] for c in CASES}
    assert len(notes) == len(CASES)                    # every note names one case
    required = ("rays", "volume", "v_lo", "v_inv_step", "bits", "g_lo", "g_inv_step", "mask", "offsets", "workspace")
    assert all(f"no {n}" in notes for n in required) and any(n.startswith("no ts_out") for n in notes)
    buffers = ("rays", "u", "tbins", "volume", "bits", "u_f", "ts_out", "sigma_c", "w_c", "mask", "offsets", "live", "workspace")
    assert all(f"misaligned {n}" in notes for n in buffers)
    assert {c["expect"] for c in CASES} == {0, EINVAL, EUNSUP}


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"{i}-{CASES[i]['note'][:40]}")
def test_abi_refusal(lib, i):
    case = CASES[i]
    assert call(lib, case) == case["expect"], (case["note"], case["args"])


def test_the_order_of_the_rules(lib):
    """On the passing side of a size limit the call gets as far as the missing ts_out (EINVAL), beyond it EUNSUP; the volume's
    and then the grid's axes are judged in front of the empty problem, the buffers behind it."""
    def f(B=4, Nc=64, Nf=128, vaxis=4, gaxis=4, ts_out=None, mask=FAKE, offsets=FAKE):
        return lib.nerf_amd_sample_pdf_volume_masked(FAKE, FAKE, FAKE, 0, 0, 0, FAKE, vaxis, 4, 4, FAKE, FAKE, FAKE, 4, gaxis, 4,
                                                     FAKE, FAKE, FAKE, ts_out, None, None, mask, offsets, None, FAKE, B, Nc, Nf,
                                                     None)
    assert f() == EINVAL
    for ok, bad in ((dict(Nc=3, Nf=1), dict(Nc=2, Nf=1)), (dict(Nc=256, Nf=256), dict(Nc=257, Nf=0)),
                    (dict(Nc=64, Nf=448), dict(Nc=64, Nf=449)), (dict(B=2 ** 32), dict(B=2 ** 32 + 1))):
        assert f(**ok) == EINVAL and f(**bad) == EUNSUP, (ok, bad)
    empty = dict(B=0, offsets=None)                    # without offsets the empty problem writes nothing
    assert f(**empty, vaxis=2, gaxis=2) == 0
    assert f(**empty, vaxis=1) == EINVAL and f(**empty, gaxis=1) == EINVAL
    assert f(**empty, mask=None, ts_out=None) == 0     # B = 0 asks for no buffer


# ---- the model -----------------------------------------------------------------------------------------------------------
def _camera_rays(oracle, synthetic, side=6):
    pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, -30, 0))).float()
    return oracle.camera_rays(pose, [side, side, synthetic.focal_from_fov(side)]).contiguous()


def _random_volume(R, seed):
    rng = np.random.default_rng(seed)
    V = (8 * rng.standard_normal(R)).astype(np.float32)
    V[rng.random(R) < 0.2] = -np.inf
    V[rng.random(R) < 0.05] = np.nan
    return V


def test_model_all_live_grid_is_the_guided_placement(oracle, synthetic):
    rays = _camera_rays(oracle, synthetic)
    B, Nc, Nf, RV, RG = rays.shape[0], 16, 24, (5, 4, 3), (4, 6, 5)
    ts_c = M.stratified(B, Nc, 1)
    u_f = torch.rand(B, Nf, generator=torch.Generator().manual_seed(2))
    V = _random_volume(RV, 0)
    v_lo, _, v_inv = G.grid_axes(RV, BOUNDS)
    g_lo, _, g_inv = OM.grid_axes(RG, ((-2, -2, -2), (2, 2, 2)))
    want = G.guided_sample(oracle, rays, ts_c, V, v_lo, v_inv, u_f)
    cells = np.ones(tuple(r - 1 for r in RG), dtype=bool)
    r = M.masked_guided_sample(oracle, rays, ts_c, V, v_lo, v_inv, cells, g_lo, g_inv, "live", u_f)
    assert torch.equal(r["ts"], want[0])
    assert torch.equal(torch.from_numpy(r["sigma_c"]), torch.from_numpy(want[1]))
    assert torch.equal(r["w_c"], want[2])
    assert r["mask"].shape == (B, 1) and np.all(r["mask"] == np.uint64((1 << (Nc + Nf)) - 1))
    assert np.array_equal(r["offsets"], np.arange(B + 1) * (Nc + Nf))


def test_model_fog_behind_a_slab_grid(oracle):
    """A uniform sigma = 0 volume tells the sampler nothing; the grid (live in cells 13 .. 18 along z only, outside empty)
    does.  With the coarse masking the pdf mass sits in the bins of the live coarse samples (measured >= 0.998 on every ray)
    and at least half of the merged samples are live (measured >= 129 of 192); without it the mass there is the live samples'
    plain share (measured <= 0.178; 19 of 192 live on the worst ray)."""
    R = (33, 33, 33)
    lo, _, inv = G.grid_axes(R, BOUNDS)
    rays = M.slab_rays()
    B, Nc, Nf = rays.shape[0], 64, 128
    assert B == 36
    ts_c = M.stratified(B, Nc, 3)
    u_f = torch.rand(B, Nf, generator=torch.Generator().manual_seed(4))
    V, cells = np.zeros(R, np.float32), M.slab_cells(R)
    r = M.masked_guided_sample(oracle, rays, ts_c, V, lo, inv, cells, lo, inv, "empty", u_f)
    live_c = r["live_c"]
    assert 0.1 < live_c.mean() < 0.2                                   # measured 14.6 %
    mass = M.live_bin_mass(r["w_c"], live_c)
    print("masked: live-bin mass min", float(mass.min()), "live per ray min", int(r["live"].sum(1).min()))
    assert torch.all(mass > 0.99), mass.min()
    assert np.all(r["live"].sum(1) >= 96), r["live"].sum(1).min()
    assert torch.all(r["w_c"][torch.from_numpy(~live_c)] == 0)
    assert np.all(np.isneginf(r["sigma_c"][~live_c])) and np.all(r["sigma_c"][live_c] == 0)
    _, _, w_plain = G.guided_sample(oracle, rays, ts_c, V, lo, inv, u_f)
    plain = M.live_bin_mass(w_plain, live_c)
    print("unmasked: live-bin mass max", float(plain.max()))
    assert torch.all(plain < 0.25), plain.max()


def test_model_all_dead_grid_gives_the_uniform_placement(oracle, synthetic):
    rays = _camera_rays(oracle, synthetic)
    B, Nc, Nf, RV, RG = rays.shape[0], 16, 24, (5, 4, 3), (4, 6, 5)
    ts_c = M.stratified(B, Nc, 1)
    u_f = torch.rand(B, Nf, generator=torch.Generator().manual_seed(2))
    v_lo, _, v_inv = G.grid_axes(RV, BOUNDS)
    g_lo, _, g_inv = OM.grid_axes(RG, BOUNDS)
    cells = np.zeros(tuple(r - 1 for r in RG), dtype=bool)
    r = M.masked_guided_sample(oracle, rays, ts_c, np.full(RV, 30.0, np.float32), v_lo, v_inv, cells, g_lo, g_inv, "empty", u_f)
    assert torch.equal(r["ts"], oracle.sample_pdf(ts_c, torch.zeros(B, Nc), u_f))
    assert np.all(np.isneginf(r["sigma_c"])) and torch.all(r["w_c"] == 0)
    assert not r["mask"].any() and not r["offsets"].any()


def test_model_ray_that_misses_the_grid_under_live(oracle):
    """Outside the grid's box every sample is live under 'live'; where the ray also misses V its weights are 0 and the
    placement is the sampler's uniform one.  A second ray through both boxes shows the other side."""
    RV, RG = (5, 4, 3), (4, 6, 5)
    v_lo, _, v_inv = G.grid_axes(RV, BOUNDS)
    g_lo, _, g_inv = OM.grid_axes(RG, BOUNDS)
    rays = torch.tensor([[0.0, 5.0, 4.0, 0.0, 0.0, -1.0],              # passes the boxes at y = 5
                         [0.1, 0.2, 4.0, 0.0, 0.0, -1.0]])             # through both
    B, Nc, Nf = 2, 16, 24
    ts_c = M.stratified(B, Nc, 5)
    u_f = torch.rand(B, Nf, generator=torch.Generator().manual_seed(6))
    cells = np.zeros(tuple(r - 1 for r in RG), dtype=bool)             # every cell dead: only the outside is live
    r = M.masked_guided_sample(oracle, rays, ts_c, np.full(RV, 30.0, np.float32), v_lo, v_inv, cells, g_lo, g_inv, "live", u_f)
    assert r["live_c"][0].all() and r["live"][0].all() and r["offsets"][1] == Nc + Nf
    assert np.all(np.isneginf(r["sigma_c"][0])) and torch.all(r["w_c"][0] == 0)
    assert torch.equal(r["ts"][0], oracle.sample_pdf(ts_c, torch.zeros(B, Nc), u_f)[0])
    assert not r["live_c"][1].all() and r["live_c"][1].any()           # live in front of and behind the box, dead inside


# ---- Python ----------------------------------------------------------------------------------------------------------------
def test_occupancy_is_keyword_only_with_default_none():
    from nerf_simple_amd import training
    from nerf_simple_amd.utils import rendering
    from nerf_simple_amd.utils.proposal import ProposalVolume
    for f in (ProposalVolume.sample, rendering.render_guided, rendering.render_guided_view, training.train_step_guided):
        p = inspect.signature(f).parameters["occupancy"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, f
        assert "terminate" not in inspect.signature(f).parameters
    p = inspect.signature(ProposalVolume.sample).parameters["return_mark"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    sig = inspect.signature(training.GraphedMaskedGuidedTrainStep.__init__).parameters
    assert list(sig)[1:9] == ["net", "optimizer", "n_rays", "Nc", "Nf", "proposal", "occupancy", "capacity"]
    assert sig["capacity"].default is inspect.Parameter.empty
    mro = training.GraphedMaskedGuidedTrainStep.__mro__
    assert mro.index(training._MaskedSteps) < mro.index(training.GraphedGuidedTrainStep)


def _host_proposal(R=(5, 4, 3)):
    """A ProposalVolume whose tensor lives on the host: enough for every refusal that comes before a launch."""
    from nerf_simple_amd.utils.proposal import ProposalVolume
    p = ProposalVolume.__new__(ProposalVolume)
    p._init(torch.full(R, float("-inf")), R, BOUNDS)
    return p


def _host_grid(R=(4, 6, 5)):
    """An OccupancyGrid whose words live on the host, likewise."""
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    words = torch.from_numpy(OM.pack_bits(np.ones(tuple(r - 1 for r in R), dtype=bool)).view(np.int32).copy())
    return OccupancyGrid(words, R, BOUNDS, "empty")


def test_python_refusals_leave_the_cpu_generator_untouched():
    from nerf_simple_amd import training
    from nerf_simple_amd.utils import rendering
    from nerf_simple_amd.utils.nets import Nerf
    prop, occ, rays = _host_proposal(), _host_grid(), torch.zeros(4, 6)
    net, small, f32 = Nerf(precision="bf16"), Nerf(6, 4, 64), Nerf(precision="fp32")      # (initialisation draws)
    gt = rays[:, :3]
    torch.manual_seed(1234)
    state = torch.get_rng_state().clone()
    Step = training.GraphedMaskedGuidedTrainStep
    refusals = (
        (TypeError, lambda: prop.sample(rays, 64, 128, occupancy=object())),                   # not a grid
        (ValueError, lambda: prop.sample(rays, 64, 128, return_mark=True)),                    # a mark needs a grid
        (RuntimeError, lambda: prop.sample(rays, 64, 128, occupancy=occ)),                     # rays on the host
        (ValueError, lambda: prop.sample(rays, 2, 8, occupancy=occ)),
        (ValueError, lambda: prop.sample(rays, 64, 449, occupancy=occ)),
        (TypeError, lambda: rendering.render_guided(rays, net, 64, 128, prop, occupancy=object())),
        (RuntimeError, lambda: rendering.render_guided(rays, small, 64, 128, prop, occupancy=occ)),
        (RuntimeError, lambda: rendering.render_guided(rays, net, 64, 128, prop, occupancy=occ)),      # grad enabled
        (TypeError, lambda: rendering.render_guided_view(net, np.eye(4), [4, 4, 4.0], 64, 128, prop, occupancy=object())),
        (TypeError, lambda: training.train_step_guided(net, None, rays, gt, 64, 128, prop, occupancy=object())),
        (RuntimeError, lambda: training.train_step_guided(f32, None, rays, gt, 64, 128, prop, occupancy=occ)),
        (RuntimeError, lambda: training.train_step_guided(small, None, rays, gt, 64, 128, prop, occupancy=occ)),
        (RuntimeError, lambda: training.train_step_guided(net, None, rays, gt, 64, 128, prop, occupancy=occ)),   # CPU rays
        (ValueError, lambda: training.train_step_guided(net, None, rays, gt, 300, 0, prop, occupancy=occ)),
        (ValueError, lambda: Step(net, None, 4, 64, 128, prop, occ, 0.5, storage="e4m3")),
        (ValueError, lambda: Step(net, None, 4, 64, 128, prop, occ, 0.5, buckets=2)),
        (TypeError, lambda: Step(net, None, 4, 64, 128, None, occ, 0.5)),
        (ValueError, lambda: Step(net, None, 4, 2, 128, prop, occ, 0.5)),
        (TypeError, lambda: Step(net, None, 4, 64, 128, prop, object(), 0.5)),
        (RuntimeError, lambda: Step(f32, None, 4, 64, 128, prop, occ, 0.5)),
        (TypeError, lambda: Step(net, None, 4, 64, 128, prop, occ)),                            # no default capacity
    )
    with torch.no_grad():
        with pytest.raises(RuntimeError):                  # under no_grad the masked render gets as far as the host rays
            rendering.render_guided(rays, net, 64, 128, prop, occupancy=occ)
    assert torch.equal(torch.get_rng_state(), state)
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
