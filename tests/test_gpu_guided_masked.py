"""The masked guided placement on the GPU (include/nerf_amd.h, "masked guided placement").  Every
comparison is exact:

  1. nerf_amd_sample_pdf_volume_masked against the chain it is defined as, all on the GPU: nerf_amd_query_points -> model
     look-up (exact) -> nerf_amd_occupancy_mark on the coarse jitter -> nerf_amd_volume_render_rays -> nerf_amd_sample_pdf ->
     nerf_amd_occupancy_mark with NERF_AMD_TS_GIVEN, in every sort bucket, scan carry, mask-word count, jitter mode and outside
     policy, through two grids whose resolution and bounds differ from the volume's, and on the slab set through the slab grid;
  2. the hot path (no optional output) against the full call, and nothing written outside the outputs; B = 0;
  3. render_guided / render_guided_view with ``occupancy=`` against the masked render on the same positions;
  4. train_step_guided(occupancy=) against render_nerf_masked on the same positions, GraphedMaskedGuidedTrainStep against it.

Inputs are judged by the numpy model BEFORE anything is launched (``informative_inputs``; these checks fail, they never skip).
occupancy_model.require_informative itself cannot hold on the slab set: every one of its 36 rays crosses the slab (so no ray is
without a live sample under 'empty'), the fullest ray has 10 live coarse samples of 64 (it asks for 16), and the merged live
fraction WITH the coarse masking is 0.70 (it asks for < 0.6; 0.70 is the point of the feature).  Its intent -- neither all nor
nothing -- is asserted clause by clause instead: a coarse live fraction inside (0.02, 0.6), dead and live merged samples on
every ray, and the fullest ray at least a quarter live after the placement."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import guided_masked_model as MM
import guided_model as G
import occupancy_graphed_model as OG
import occupancy_model as OM
from test_gpu_guided import Lib, make_rays, make_volume
from test_gpu_occupancy_graphed import compare_gradients

pytestmark = pytest.mark.gpu

BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))            # of the volumes
VOLUMES = ((5, 4, 3), (33, 17, 9))
# merged counts 4, 192, 131, 259, 512: a partial last mask word, whole words, the sort's buckets, the scan's chunk carries
SIZES = ((3, 1), (64, 128), (66, 65), (130, 129), (256, 256))
MODES = ("u", "ts", "rng", "rng+seed_in_memory")
OUTSIDE = ("live", "empty")
# two grids that share neither resolution nor bounds with the volumes; the ball's radius and the mask's seed are chosen (on
# the CPU, informative_inputs) so that the 37 rays hold a ray without a live coarse sample and a fully live ray
GRID_BOUNDS = ((-4.5, -4.2, -4.8), (4.5, 4.8, 4.2))
BALL = dict(R=(41, 37, 33), radius=1.0)
RANDOM = dict(R=(4, 5, 3), seed=34)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def bits(t_):
    t_ = t_.contiguous()
    return t_.view(torch.int32) if t_.dtype == torch.float32 else t_


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def grid_cells(name):
    if name == "ball":
        return OM.ball_cells(BALL["R"], GRID_BOUNDS, BALL["radius"]), BALL["R"], GRID_BOUNDS
    if name == "random":
        C = tuple(r - 1 for r in RANDOM["R"])
        return np.random.default_rng(RANDOM["seed"]).random(C) < 0.5, RANDOM["R"], GRID_BOUNDS
    return MM.slab_cells(), (33, 33, 33), BOUNDS


def host_jitter(B, Nc, Nf, seed):
    """(tbins, u_c, ts_c, u_f) on the host, the draws of test_gpu_guided.jitter_args"""
    g = torch.Generator().manual_seed(seed)
    tbins = torch.linspace(2, 6, Nc + 1)
    u_c = torch.rand(B, Nc, generator=g)
    u_f = torch.rand(B, max(Nf, 1), generator=g)[:, :Nf].contiguous()
    return tbins, u_c, ((tbins[1] - tbins[0]) * u_c + tbins[:-1]).contiguous(), u_f


def jitter_args(L, mode, B, Nc, Nf, seed, ts_c=None, u_f=None):
    """The kernel's jitter arguments and the same for the chain's own calls (test_gpu_guided.jitter_args, with the coarse
    positions and the fine uniforms optionally given: the slab set's)."""
    _lib, dev = L._lib, L.dev
    tbins, u_c, ts_host, u_f_host = host_jitter(B, Nc, Nf, seed)
    tbins, u_c = tbins.to(dev), u_c.to(dev)
    u_f = (u_f_host if u_f is None else u_f).to(dev)
    RNG, MEM, GIVEN = _lib.FLAG_DEVICE_RNG, _lib.FLAG_SEED_IN_MEMORY, _lib.FLAG_TS_GIVEN
    s0, k = 987654321, 5
    if mode == "u":
        return dict(jit=L.ptr(u_c), tbins=tbins, flags=0, seed=0, u_f=u_f, keep=u_c, q=(L.ptr(u_c), tbins, 0, 0), pdf=(0, 0))
    if mode == "ts":
        ts = (ts_host if ts_c is None else ts_c).contiguous().to(dev)
        return dict(jit=L.ptr(ts), tbins=None, flags=GIVEN, seed=0, u_f=u_f, keep=ts, q=(L.ptr(ts), None, GIVEN, 0), pdf=(0, 0))
    if mode == "rng":
        return dict(jit=None, tbins=tbins, flags=RNG, seed=s0, u_f=None, keep=None, q=(None, tbins, RNG, s0), pdf=(RNG, s0))
    off = torch.tensor([k], dtype=torch.int64, device=dev)
    return dict(jit=L.ptr(off), tbins=tbins, flags=RNG | MEM, seed=s0, u_f=None, keep=off,
                q=(None, tbins, RNG, s0 + k), pdf=(RNG, s0 + k))


class MLib(Lib):
    """test_gpu_guided.Lib plus the mark and the new entry point."""

    def h3(self, a):
        return (ctypes.c_float * 3)(*[float(x) for x in a])

    def grid(self, name):
        """(cells, words on the device, R, lo, inv_step) of a named grid"""
        cells, R, bounds = grid_cells(name)
        lo, _, inv = OM.grid_axes(R, bounds)
        words = torch.from_numpy(OM.pack_bits(cells).view(np.int32).copy()).to(self.dev)
        return cells, words, R, lo, inv

    def workspace(self, B):
        return torch.empty(max(int(self.lib.nerf_amd_occupancy_workspace_bytes(B)), 256), dtype=torch.uint8, device=self.dev)

    def mark(self, rays, jit, tbins, flags, seed, rid, words, R, lo, inv, B, N):
        i64 = dict(dtype=torch.int64, device=self.dev)
        mask, offsets, live = torch.empty(B, (N + 63) // 64, **i64), torch.empty(B + 1, **i64), torch.empty(1, **i64)
        ws = self.workspace(B)
        self._lib.check(self.lib.nerf_amd_occupancy_mark(
            self.ptr(rays), jit, self.ptr(tbins), flags, seed, rid, self.ptr(words), *R, self.h3(lo), self.h3(inv), self.ptr(mask),
            self.ptr(offsets), self.ptr(live), self.ptr(ws), B, N, self.st()), "occupancy_mark")
        return mask, offsets, live

    def masked(self, rays, jit, tbins, flags, seed, rid, vol, v_lo, v_inv, words, R, g_lo, g_inv, u_f, ts_out, sigma_c, w_c, mask,
               offsets, live, ws, B, Nc, Nf):
        p = lambda x: self.ptr(x) if torch.is_tensor(x) else x
        return self.lib.nerf_amd_sample_pdf_volume_masked(
            self.ptr(rays), jit, self.ptr(tbins), flags, seed, rid, self.ptr(vol), *vol.shape, self.h3(v_lo), self.h3(v_inv),
            self.ptr(words), *R, self.h3(g_lo), self.h3(g_inv), self.ptr(u_f), p(ts_out), p(sigma_c), p(w_c), p(mask), p(offsets),
            p(live), p(ws), B, Nc, Nf, self.st())


def unpack(mask, N):
    """mask words int64 [B, W] (device) -> bool [B, N] (numpy)"""
    m = mask.cpu().numpy().view(np.uint64)
    b = (m[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return b.reshape(m.shape[0], -1)[:, :N].astype(bool)


def chain(L, rays, a, rid, V, vol_lo, vol_inv, grid, oflag, B, Nc, Nf):
    """The six steps through the existing entry points -> (ts, sigma_c, w_c, mask, offsets, live) on the device."""
    _, words, R, g_lo, g_inv = grid
    qj, qtb, qflags, qseed = a["q"]
    q, ts_c = L.query_points(rays, qj, qtb, qflags, qseed, rid, B, Nc)                                            # 1
    value = G.lookup(q[:, :3].cpu().numpy().reshape(B, Nc, 3), V, vol_lo, vol_inv)                                # 2
    mask_c, _, _ = L.mark(rays, a["jit"], a["tbins"], a["flags"] | oflag, a["seed"], rid, words, R, g_lo, g_inv, B, Nc)   # 3
    sigma = torch.from_numpy(np.where(unpack(mask_c, Nc), value, np.float32(-np.inf)).astype(np.float32)).to(L.dev)
    w = L.weights(sigma, ts_c, rays)                                                                              # 4
    ts = L.sample_pdf(ts_c, w, a["u_f"], a["pdf"][0], a["pdf"][1], rid, Nf)                                       # 5
    mask, offsets, live = L.mark(rays, L.ptr(ts), None, L._lib.FLAG_TS_GIVEN | oflag, 0, 0, words, R, g_lo, g_inv, B, Nc + Nf)
    return ts, sigma, w, mask, offsets, live                                                                      # 6


def entry_point(L, rays, a, rid, vol, vol_lo, vol_inv, grid, oflag, B, Nc, Nf, fill=float("nan")):
    _, words, R, g_lo, g_inv = grid
    N = Nc + Nf
    ts_out, sigma_c, w_c = (torch.full(s_, fill, **L.f32) for s_ in ((B, N), (B, Nc), (B, Nc)))
    i64 = dict(dtype=torch.int64, device=L.dev)
    mask, offsets, live = torch.full((B, (N + 63) // 64), -1, **i64), torch.full((B + 1,), -1, **i64), torch.full((1,), -1, **i64)
    rc = L.masked(rays, a["jit"], a["tbins"], a["flags"] | oflag, a["seed"], rid, vol, vol_lo, vol_inv, words, R, g_lo, g_inv,
                  a["u_f"], ts_out, sigma_c, w_c, mask, offsets, live, L.workspace(B), B, Nc, Nf)
    assert rc == 0, rc
    return ts_out, sigma_c, w_c, mask, offsets, live


# ---- the inputs, judged on the CPU before anything is launched ----------------------------------------------------------------
_judged = {}


def informative_inputs(oracle):
    """The numpy model's verdict on the inputs of test 1 at (64, 128), explicit jitter: per (grid, outside) of the 37-ray set a
    ray with no live coarse sample and a fully live ray; the slab set neither all nor nothing (module docstring)."""
    if _judged:
        return _judged
    Nc, Nf, R = 64, 128, VOLUMES[1]
    V = make_volume(R, 99)
    v_lo, _, v_inv = G.grid_axes(R, BOUNDS)
    rays = make_rays(37, 137)
    _, _, ts_c, u_f = host_jitter(37, Nc, Nf, 1000 * Nc + Nf + 37)
    for name in ("ball", "random"):
        cells, RG, gb = grid_cells(name)
        g_lo, _, g_inv = OM.grid_axes(RG, gb)
        assert RG != R and gb != BOUNDS and 0.0 < cells.mean() < 1.0
        for outside in OUTSIDE:
            r = MM.masked_guided_sample(oracle, rays, ts_c, V, v_lo, v_inv, cells, g_lo, g_inv, outside, u_f)
            none, full = ~r["live_c"].any(1), r["live"].all(1)
            assert none.any(), f"{name}/{outside}: no ray without a live coarse sample"
            assert full.any(), f"{name}/{outside}: no fully live ray"
            assert 0.02 < r["live"].mean() < 0.98, (name, outside, r["live"].mean())
            _judged[(name, outside)] = (int(none.sum()), int(full.sum()), float(r["live"].mean()))
    rays = MM.slab_rays()
    cells, RG, gb = grid_cells("slab")
    g_lo, _, g_inv = OM.grid_axes(RG, gb)
    ts_c, u_f = MM.stratified(36, Nc, 3), torch.rand(36, Nf, generator=torch.Generator().manual_seed(4))
    for outside in OUTSIDE:
        r = MM.masked_guided_sample(oracle, rays, ts_c, V, v_lo, v_inv, cells, g_lo, g_inv, outside, u_f)
        fc, fm = OM.stats(r["live_c"]), OM.stats(r["live"])
        assert 0.02 < fc[0] < 0.6, (outside, fc)                                  # require_informative's fraction clause
        assert r["live_c"].any(1).all() and not r["live_c"].all(1).any(), outside    # every ray crosses the slab and leaves it
        assert r["live"].any(1).all() and not r["live"].all(1).any(), outside      # the merged masks: neither all nor nothing
        assert fm[1] >= -(-(Nc + Nf) // 4), (outside, fm)                          # ... and its fullest-ray clause, merged
        _judged[("slab", outside)] = (fc, fm)
    return _judged


def test_the_inputs_are_informative(oracle):
    for key, v in informative_inputs(oracle).items():
        print(key, v)


# ---- 1. the entry point against the six launches -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def volumes(dev):
    out = []
    for R in VOLUMES:
        V = make_volume(R, 99 if R == VOLUMES[1] else sum(R))
        lo, _, inv = G.grid_axes(R, BOUNDS)
        out.append((V, torch.from_numpy(V).to(dev), lo, inv))
    return out


def compare(got, want, tag):
    for name, g, w in zip(("ts_out", "sigma_c", "w_c", "mask", "offsets", "live"), got, want):
        assert same(g, w), (name,) + tag


@pytest.mark.parametrize("outside", OUTSIDE)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_entry_point_equals_the_chain(dev, oracle, volumes, Nc, Nf, mode, outside):
    informative_inputs(oracle)
    L = MLib(dev)
    oflag = L._lib.FLAG_OUTSIDE_EMPTY if outside == "empty" else 0
    rid, N = 17, Nc + Nf
    seen_dead = seen_live = seen_inf = False
    for gname in ("ball", "random"):
        grid = L.grid(gname)
        for V, vol, v_lo, v_inv in volumes:
            for B in (1, 5, 37):
                rays = make_rays(B, 100 + B).to(dev)
                a = jitter_args(L, mode, B, Nc, Nf, 1000 * Nc + Nf + B)
                want = chain(L, rays, a, rid, V, v_lo, v_inv, grid, oflag, B, Nc, Nf)
                got = entry_point(L, rays, a, rid, vol, v_lo, v_inv, grid, oflag, B, Nc, Nf)
                torch.cuda.synchronize(dev)
                tag = (gname, tuple(vol.shape), B, Nc, Nf, mode, outside)
                compare(got, want, tag)
                ts, sigma_c, _, mask, offsets, live = got
                assert bool(torch.all(ts[:, 1:] >= ts[:, :-1])), tag
                lv = unpack(mask, N)
                assert np.array_equal(offsets.cpu().numpy(), OM.offsets(lv)) and int(live) == int(lv.sum()), tag
                if N % 64:                                               # the padding bits of the last word are zero
                    assert not bool((mask[:, -1] >> (N % 64)).any()), tag
                seen_dead |= bool((~lv).any()); seen_live |= bool(lv.any()); seen_inf |= bool(torch.isneginf(sigma_c).any())
    assert seen_dead and seen_live and seen_inf


@pytest.mark.parametrize("outside", OUTSIDE)
@pytest.mark.parametrize("mode", MODES)
def test_slab_set_through_the_slab_grid(dev, oracle, volumes, mode, outside):
    """The 36 rays of the fog case with its coarse positions (generator seed 3) and fine uniforms (seed 4) where the mode takes
    them, through the slab grid, over both volumes; with explicit positions the numpy model predicts the masks too."""
    informative_inputs(oracle)
    L = MLib(dev)
    oflag = L._lib.FLAG_OUTSIDE_EMPTY if outside == "empty" else 0
    B, Nc, Nf, rid = 36, 64, 128, 0
    rays_h = MM.slab_rays()
    rays, grid = rays_h.to(dev), L.grid("slab")
    ts_c, u_f = MM.stratified(B, Nc, 3), torch.rand(B, Nf, generator=torch.Generator().manual_seed(4))
    a = jitter_args(L, mode, B, Nc, Nf, 0, ts_c=ts_c, u_f=u_f)
    for V, vol, v_lo, v_inv in volumes:
        want = chain(L, rays, a, rid, V, v_lo, v_inv, grid, oflag, B, Nc, Nf)
        got = entry_point(L, rays, a, rid, vol, v_lo, v_inv, grid, oflag, B, Nc, Nf)
        torch.cuda.synchronize(dev)
        compare(got, want, (tuple(vol.shape), mode, outside))
        if mode == "ts":
            r = MM.masked_guided_sample(oracle, rays_h, ts_c, V, v_lo, v_inv, grid[0], grid[3], grid[4], outside, u_f)
            assert np.array_equal(got[1].cpu().numpy().view(np.int32), r["sigma_c"].view(np.int32))
            assert bool(torch.all(got[2].cpu()[torch.from_numpy(~r["live_c"])] == 0))
            assert np.array_equal(unpack(got[3], Nc + Nf), r["live"]) and np.array_equal(got[4].cpu().numpy(), r["offsets"])


def test_all_live_grid_is_the_guided_placement(dev, volumes):
    L = MLib(dev)
    V, vol, v_lo, v_inv = volumes[1]
    B, Nc, Nf, rid = 37, 66, 65, 3
    R = (4, 6, 5)
    g_lo, _, g_inv = OM.grid_axes(R, GRID_BOUNDS)
    cells = np.ones(tuple(r - 1 for r in R), dtype=bool)
    words = torch.from_numpy(OM.pack_bits(cells).view(np.int32).copy()).to(dev)
    rays = make_rays(B, 137).to(dev)
    a = jitter_args(L, "rng", B, Nc, Nf, 1)
    ts, sigma_c, w_c, mask, offsets, live = entry_point(L, rays, a, rid, vol, v_lo, v_inv, (cells, words, R, g_lo, g_inv), 0, B, Nc, Nf)
    want = [torch.empty(s_, **L.f32) for s_ in ((B, Nc + Nf), (B, Nc), (B, Nc))]
    L.guided(rays, a["jit"], a["tbins"], a["flags"], a["seed"], rid, vol, v_lo, v_inv, a["u_f"], *want, B, Nc, Nf)
    torch.cuda.synchronize(dev)
    assert same(ts, want[0]) and same(sigma_c, want[1]) and same(w_c, want[2])
    full = torch.tensor([-1, -1, (1 << 3) - 1], dtype=torch.int64, device=dev).expand(B, 3)       # 131 = 64 + 64 + 3 bits
    assert same(mask, full.contiguous()) and int(live) == B * (Nc + Nf)
    assert torch.equal(offsets.cpu(), torch.arange(B + 1) * (Nc + Nf))


# ---- 2. the hot path, B = 0 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc,Nf", ((64, 128), (66, 65)))
def test_hot_path_writes_the_same_outputs_and_nothing_else(dev, volumes, Nc, Nf):
    L = MLib(dev)
    V, vol, v_lo, v_inv = volumes[1]
    _, words, R, g_lo, g_inv = L.grid("ball")
    B, PAD, S, N = 37, 64, -12345.0, Nc + Nf
    W = (N + 63) // 64
    rays = make_rays(B, 31).to(dev)
    a = jitter_args(L, "rng", B, Nc, Nf, 3)
    oflag = L._lib.FLAG_OUTSIDE_EMPTY

    def padded(n, dtype):
        return torch.full((PAD + n + PAD,), S, dtype=dtype, device=dev)

    def inner(b):
        return ctypes.c_void_p(b.data_ptr() + b.element_size() * PAD)

    sizes = ((B * N, torch.float32), (B * Nc, torch.float32), (B * Nc, torch.float32), (B * W, torch.int64), (B + 1, torch.int64),
             (1, torch.int64))
    full = [padded(n, dt) for n, dt in sizes]
    hot = [padded(n, dt) for n, dt in (sizes[0], sizes[3], sizes[4])]
    args = (rays, a["jit"], a["tbins"], a["flags"] | oflag, a["seed"], 9, vol, v_lo, v_inv, words, R, g_lo, g_inv, a["u_f"])
    assert L.masked(*args, *[inner(b) for b in full], L.workspace(B), B, Nc, Nf) == 0
    for _ in range(2):                                                   # and again: the same bytes
        assert L.masked(*args, inner(hot[0]), None, None, inner(hot[1]), inner(hot[2]), None, L.workspace(B), B, Nc, Nf) == 0
    torch.cuda.synchronize(dev)
    for b in full + hot:
        assert bool(torch.all(b[:PAD] == S)) and bool(torch.all(b[-PAD:] == S))
    for b in (full[0], full[1], full[2], hot[0]):
        assert not bool(torch.any(b[PAD:-PAD] == S))
    for h, f in zip(hot, (full[0], full[3], full[4])):
        assert same(h[PAD:-PAD], f[PAD:-PAD])
    assert int(full[5][PAD]) == int(full[4][PAD + B]) > 0


def test_empty_problem(dev, volumes):
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    from nerf_simple_amd.utils.proposal import ProposalVolume
    L = MLib(dev)
    V, vol, v_lo, v_inv = volumes[0]
    cells, words, R, g_lo, g_inv = L.grid("random")
    i64 = dict(dtype=torch.int64, device=dev)
    offsets, live = torch.full((1,), 7, **i64), torch.full((1,), 7, **i64)
    tbins = torch.linspace(2, 6, 65).to(dev)                             # the jitter rule is judged in front of the empty problem
    rc = L.masked(None, None, tbins, L._lib.FLAG_DEVICE_RNG, 0, 0, vol, v_lo, v_inv, words, R, g_lo, g_inv, None, None, None, None,
                  None, offsets, live, L.workspace(0), 0, 64, 128)
    torch.cuda.synchronize(dev)
    assert rc == 0 and int(offsets) == 0 and int(live) == 0
    prop = ProposalVolume.from_sigma(vol, BOUNDS)
    occ = OccupancyGrid.from_mask(torch.from_numpy(cells).to(dev), GRID_BOUNDS, outside="empty")
    ts, mark = prop.sample(torch.empty(0, 6, **L.f32), 16, 24, device_rng=True, occupancy=occ, return_mark=True)
    assert ts.shape == (0, 40) and mark.live == 0 and mark.mask.shape == (0, 1) and mark.offsets.tolist() == [0]


# ---- 3. the renders ------------------------------------------------------------------------------------------------------------
NAMES = ("rgb", "disp", "alpha", "acc", "w", "ts")


@pytest.fixture(scope="module")
def scene(dev, oracle, synthetic):
    """A structured network, its proposal volume at 33^3, a ball grid of other resolution and bounds, 37 camera rays."""
    import occupancy_hierarchical_model as H
    from nerf_simple_amd.utils.nets import Nerf
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    from nerf_simple_amd.utils.proposal import ProposalVolume
    net = Nerf(precision="bf16").to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, "structured"))
    prop = ProposalVolume(33, BOUNDS, device=dev).update(net)
    RG, gb = (29, 25, 21), ((-1.4, -1.3, -1.2), (1.2, 1.3, 1.4))
    occ = OccupancyGrid.from_mask(torch.from_numpy(OM.ball_cells(RG, gb, 0.9)).to(dev), gb, outside="empty")
    ones = torch.ones((7, 6, 5), dtype=torch.bool, device=dev)
    all_live = OccupancyGrid.from_mask(ones, gb, outside="live")
    rays, gt, u_c, u_f = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, 37, 16, 24))
    return dict(net=net, prop=prop, occ=occ, all_live=all_live, rays=rays, gt=gt, u_c=u_c, u_f=u_f, Nc=16, Nf=24)


@pytest.mark.parametrize("precision", ("fp16", "bf16", "fp32"))
def test_render_guided_masked_is_the_masked_render_on_its_positions(dev, scene, precision):
    from nerf_simple_amd.utils.rendering import render_guided, render_nerf
    s = scene
    Nc, Nf, occ = s["Nc"], s["Nf"], s["occ"]
    kw = dict(u_c=s["u_c"], u_f=s["u_f"])
    with torch.no_grad():
        occ.last_stats = None
        out = render_guided(s["rays"], s["net"], Nc, Nf, s["prop"], precision=precision, occupancy=occ, **kw)
        stats = occ.last_stats
        assert len(out) == 6
        ts, mark = s["prop"].sample(s["rays"], Nc, Nf, occupancy=occ, return_mark=True, **kw)
        assert stats["rays"] == 37 and stats["samples"] == 37 * (Nc + Nf) and stats["live"] == mark.live
        assert 0 < mark.live < 37 * (Nc + Nf) and mark.N == Nc + Nf and mark.B == 37
        want = render_nerf(s["rays"], s["net"], Nc + Nf, ts=ts, precision=precision, occupancy=occ) + (ts,)
        assert occ.last_stats == stats
        for name, a, b in zip(NAMES, out, want):
            assert same(a, b), (precision, name)
        # the coarse masking moved the positions: not the unmasked placement's
        assert not same(ts, s["prop"].sample(s["rays"], Nc, Nf, **kw))
        # an all-live grid: the dense guided render, all six outputs
        got = render_guided(s["rays"], s["net"], Nc, Nf, s["prop"], precision=precision, occupancy=s["all_live"], **kw)
        dense = render_guided(s["rays"], s["net"], Nc, Nf, s["prop"], precision=precision, **kw)
        assert s["all_live"].last_stats["live"] == 37 * (Nc + Nf)
        for name, a, b in zip(NAMES, got, dense):
            assert same(a, b), (precision, name, "all live")


def test_render_guided_view_masked_is_its_composition(dev, scene):
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils.rendering import generate_rays, render_guided_view, render_nerf
    s = scene
    pose = np.eye(4, dtype=np.float32)
    pose[2, 3] = 4.0
    cam = (6, 7, 9.0)
    Nc, Nf, occ = s["Nc"], s["Nf"], s["occ"]
    with torch.no_grad():
        got = render_guided_view(s["net"], pose, cam, Nc, Nf, s["prop"], device_rng=True, seed=21, precision="fp16", occupancy=occ)
        stats = occ.last_stats
        rays = generate_rays(pose, cam, dev)
        ts, mark = s["prop"].sample(rays, Nc, Nf, device_rng=True, seed=21, ray_id0=0, occupancy=occ, return_mark=True)
        assert stats["live"] == mark.live and 0 < mark.live < 42 * (Nc + Nf)
        # nerf_amd_volume_render_masked_pixels on the network's output at the live points of this mark
        pts = torch.empty((mark.live, 6), dtype=torch.float32, device=dev)
        lib, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
        _lib.check(lib.nerf_amd_occupancy_points(ptr(rays), ptr(ts), None, _lib.FLAG_TS_GIVEN, 0, 0, ptr(mark.mask),
                                                 ptr(mark.offsets), ptr(pts), mark.live, 42, Nc + Nf, st), "points")
        raw = torch.empty((mark.live, 4), dtype=torch.float32, device=dev)
        _lib.check(lib.nerf_amd_mlp_forward(ptr(pts), ptr(s["net"].packed_weights(_lib.FP16)), ptr(raw), mark.live, _lib.FP16, st),
                   "forward")
        px = torch.empty((42, 4), dtype=torch.float32, device=dev)
        _lib.check(lib.nerf_amd_volume_render_masked_pixels(ptr(raw), ptr(rays), ptr(ts), None, _lib.FLAG_TS_GIVEN, 0, 0,
                                                            ptr(mark.mask), ptr(mark.offsets), ptr(px), 42, Nc + Nf, st), "pixels")
        assert same(got, px)
        rgb, disp, _, _, _ = render_nerf(rays, s["net"], Nc + Nf, ts=ts, precision="fp16", occupancy=occ)
        assert same(got, torch.cat([rgb.clamp(0., 1.), disp[:, None]], dim=1))
        part = render_guided_view(s["net"], pose, cam, Nc, Nf, s["prop"], device_rng=True, seed=21, precision="fp16", ray0=11,
                                  n_rays=20, occupancy=occ)
        assert same(part, got[11:31])                                    # keyed by global pixel id


# ---- 4. training -----------------------------------------------------------------------------------------------------------------
def _net(dev, synthetic):
    from nerf_simple_amd.utils.nets import Nerf
    net = Nerf(precision="bf16").to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, "default"))
    return net


def _grads(net):
    return {k: p.grad.clone() for k, p in net.named_parameters()}


def test_train_step_guided_masked_is_the_masked_render_on_its_positions(dev, scene, synthetic):
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import mse_loss, render_nerf_masked, train_step_guided
    s = scene
    Nc, Nf, occ = s["Nc"], s["Nf"], s["occ"]
    a, b = _net(dev, synthetic), _net(dev, synthetic)
    kw = dict(u_c=s["u_c"], u_f=s["u_f"])
    loss = train_step_guided(a, FusedAdam(a, lr=0.0), s["rays"], s["gt"], Nc, Nf, s["prop"], occupancy=occ, **kw)
    stats = occ.last_stats
    ts = loss.ts
    assert not ts.requires_grad and same(ts, s["prop"].sample(s["rays"], Nc, Nf, occupancy=occ, **kw))
    opt_b = FusedAdam(b, lr=0.0)
    opt_b.zero_grad(set_to_none=True)
    want = mse_loss(render_nerf_masked(s["rays"], b, Nc + Nf, occ, ts=ts)[0], s["gt"])
    want.backward()
    assert occ.last_stats == stats and 0 < stats["live"] < 37 * (Nc + Nf) and stats["network_launches"] == 1
    assert same(loss, want.detach()), (float(loss), float(want))
    compare_gradients(_grads(a), _grads(b), "eager masked guided step")
    assert any(bool((p.grad != 0).any()) for p in a.parameters())
    assert not s["prop"].sigma.requires_grad and s["prop"].sigma.grad is None


def _graphed_inputs(dev, oracle, synthetic, B, Nc, Nf):
    import occupancy_hierarchical_model as H
    rays, gt, _, _ = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, B, Nc, Nf))
    return rays, gt


def test_graphed_masked_guided_step(dev, synthetic, oracle):
    """256 rays x (16 + 16), device_rng=True, lr = 0 (the reason: test_gpu_guided.test_graphed_guided_step), three replays
    against the eager masked guided step with seed + k; the grid is updated in place behind replay 1, the volume behind
    replay 2; nerf_amd_occupancy_mark is not among the captured launches."""
    from nerf_simple_amd import training
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.utils.occupancy import TrainingOccupancyGrid
    from nerf_simple_amd.utils.proposal import ProposalVolume
    B, Nc, Nf, seed, rid = 256, 16, 16, 400, 7
    N = Nc + Nf
    rays, gt = _graphed_inputs(dev, oracle, synthetic, B, Nc, Nf)
    net, twin = _net(dev, synthetic), _net(dev, synthetic)
    structured = _net(dev, synthetic)
    structured.load_state_dict(synthetic.synthetic_state_dict(0, "structured"))
    prop = ProposalVolume(17, BOUNDS, device=dev)
    occ = TrainingOccupancyGrid((25, 21, 19), ((-1.4, -1.3, -1.2), (1.2, 1.3, 1.4)), outside="empty", device=dev)
    launched = []
    real = training._launch
    training._launch = lambda name, *args: (launched.append(name), real(name, *args))[1]
    try:
        stepper = training.GraphedMaskedGuidedTrainStep(net, FusedAdam(net, lr=0.0), B, Nc, Nf, prop, occ, 1.0, device_rng=True,
                                                        seed=seed, ray_id0=rid)
    finally:
        training._launch = real
    assert "nerf_amd_sample_pdf_volume_masked" in launched and "nerf_amd_occupancy_mark" not in launched
    assert "nerf_amd_sample_pdf_volume" not in launched and "nerf_amd_occupancy_points_capped" in launched
    assert stepper.capacity == B * N
    opt_twin = FusedAdam(twin, lr=0.0)
    lives = []
    for k in (1, 2, 3):
        if k == 2:                                                      # in place, between two replays
            level = float(np.percentile(training_density(structured, occ).cpu().numpy(), 80))
            ptr0 = occ.words.data_ptr()
            occ.update(structured, level, decay=0.5, dilate=1)
            assert occ.words.data_ptr() == ptr0 and 0.0 < occ.cell_fraction < 1.0
        if k == 3:
            prop.update(structured)
        loss = stepper.step(rays, gt).clone()
        ts_f = stepper.ts_f.clone()
        counts = stepper.counts()
        want = training.train_step_guided(twin, opt_twin, rays, gt, Nc, Nf, prop, device_rng=True, seed=seed + k, ray_id0=rid,
                                          occupancy=occ)
        live = occ.last_stats["live"]
        assert counts == {"step": k, "samples": B * N, "live": live, "kept": live, "capacity": B * N}, k
        assert same(loss, want), (k, float(loss), float(want))
        assert same(ts_f, want.ts), k
        compare_gradients(_grads(net), _grads(twin), ("graphed masked guided step", k))
        lives.append(live)
    assert lives[1] < lives[0] and 0 < lives[2] < B * N and stepper.overflow_steps == 0
    # both addresses are baked into the graph
    keep = occ.words
    occ.words = occ.words.clone()
    with pytest.raises(RuntimeError, match="words"):
        stepper.step(rays, gt)
    occ.words = keep
    prop.sigma = prop.sigma.clone()
    with pytest.raises(RuntimeError, match="replaced"):
        stepper.step(rays, gt)
    assert stepper.opt.step_count == 3


def training_density(net, occ):
    from nerf_simple_amd.utils import mesh
    return mesh.density_grid(net, occ.resolution, occ.bounds)


def test_short_capacity_is_the_eager_step_under_mask_C_and_is_reported(dev, synthetic, oracle):
    from nerf_simple_amd import _lib, training
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    from nerf_simple_amd.utils.proposal import ProposalVolume
    B, Nc, Nf, seed, rid = 256, 16, 16, 400, 7
    N = Nc + Nf
    rays, gt = _graphed_inputs(dev, oracle, synthetic, B, Nc, Nf)
    structured = _net(dev, synthetic)
    structured.load_state_dict(synthetic.synthetic_state_dict(0, "structured"))
    prop = ProposalVolume(17, BOUNDS, device=dev).update(structured)
    gb = ((-1.4, -1.3, -1.2), (1.2, 1.3, 1.4))
    occ = OccupancyGrid.from_mask(torch.from_numpy(OM.ball_cells((25, 21, 19), gb, 0.9)).to(dev), gb, outside="empty")
    # the eager placement of step 1 and its mark
    ts, mark = prop.sample(rays, Nc, Nf, device_rng=True, seed=seed + 1, ray_id0=rid, occupancy=occ, return_mark=True)
    live = unpack(mark.mask, N)
    total = int(live.sum())
    assert total == mark.live and 0.02 < total / (B * N) < 0.98
    C = -(-total // 2)
    assert C not in set(OM.offsets(live).tolist())                       # the capacity cuts inside a ray
    kept = OG.mask_C(live, C)
    twin = _net(dev, synthetic)
    pts = torch.empty((total, 6), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().nerf_amd_occupancy_points(_lib.ptr(rays), _lib.ptr(ts), None, _lib.FLAG_TS_GIVEN, 0, 0, _lib.ptr(mark.mask),
                                                    _lib.ptr(mark.offsets), _lib.ptr(pts), total, B, N, _lib.stream_ptr(dev)),
               "points")
    mask_c = torch.from_numpy(OM.mask_words(kept).view(np.int64).copy()).to(dev)
    offsets_c = torch.from_numpy(OM.offsets(kept)).to(dev)
    params = [p for _, p in twin.named_parameters()]
    raw, _ = training._FusedDense.apply(twin, None, None, None, 0, 0, 0, 1, pts[:C].contiguous(), *params)
    head = (rays, ts, None, _lib.FLAG_TS_GIVEN, 0, 0, mask_c, offsets_c)
    want = training.mse_loss(training._MaskedVolumeRender.apply(raw.reshape(-1, 4), head, B, N)[0], gt)
    want.backward()
    full = training.mse_loss(training.render_nerf_masked(rays, _net(dev, synthetic), N, occ, ts=ts)[0], gt)
    net = _net(dev, synthetic)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        stepper = training.GraphedMaskedGuidedTrainStep(net, FusedAdam(net, lr=0.0), B, Nc, Nf, prop, occ, C, device_rng=True,
                                                        seed=seed, ray_id0=rid, check_every=1)
        loss = stepper.step(rays, gt).clone()
    assert same(stepper.ts_f, ts)
    assert same(loss, want.detach()), (float(loss), float(want))
    assert not same(loss, full.detach())                                  # the dropped tail did matter
    compare_gradients(_grads(net), _grads(twin), "short capacity")
    assert stepper.last_stats is None and stepper.overflow_steps == 0     # nothing polled yet
    torch.cuda.synchronize()
    with pytest.warns(RuntimeWarning, match=rf"step 1 had {total} live samples for a capacity of {C} points"):
        stepper.step(rays, gt)
    assert stepper.overflow_steps == 1
    assert stepper.last_stats == {"step": 1, "samples": B * N, "live": total, "kept": C, "capacity": C}


def test_all_dead_batch(dev, synthetic, oracle):
    from nerf_simple_amd import training
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.utils.occupancy import OccupancyGrid
    from nerf_simple_amd.utils.proposal import ProposalVolume
    B, Nc, Nf = 256, 16, 16
    N = Nc + Nf
    rays, gt = _graphed_inputs(dev, oracle, synthetic, B, Nc, Nf)
    away = torch.cat([rays[:, :3], -rays[:, 3:]], 1).contiguous()        # the camera looks away from the grid
    prop = ProposalVolume(17, BOUNDS, device=dev)
    gb = ((-1.4, -1.3, -1.2), (1.2, 1.3, 1.4))
    occ = OccupancyGrid.from_mask(torch.from_numpy(OM.ball_cells((25, 21, 19), gb, 0.9)).to(dev), gb, outside="empty")
    net = _net(dev, synthetic)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        stepper = training.GraphedMaskedGuidedTrainStep(net, FusedAdam(net, lr=0.0), B, Nc, Nf, prop, occ, 0.25, device_rng=True)
        loss = stepper.step(away, gt).clone()
        assert stepper.capacity == B * N // 4
        assert stepper.counts() == {"step": 1, "samples": B * N, "live": 0, "kept": 0, "capacity": B * N // 4}
    want = float((gt.double() ** 2).mean())
    assert np.isfinite(float(loss)) and abs(float(loss) - want) <= 1e-6 * want, (float(loss), want)
    for k, p in net.named_parameters():
        assert bool((p.grad == 0).all()), k
