"""Background and sigma noise for the coarse + fine pair on the GPU (csrc/composite_pair.hip, csrc/occupancy_train.hip,
training.train_step_hierarchical / GraphedHierarchicalTrainStep / GraphedMaskedHierarchicalTrainStep and
rendering.render_hierarchical[_view] with ``controls=``).

Kernel level: the two coarse heads against THEIR DEFINITION, the chain of the public entry points (include/nerf_amd.h) with
nerf_amd_sample_pdf on the chain's w, bit for bit; the masked one under mask_C / offsets_C at three capacities, against the dense
one on an all-live grid, on an all-dead batch and under std = 1e30; one case per head against float64 by the rule and the
constants of tests/background_model.py.  Step level: the eager pair step against the public renders composed by hand with the two
noise seeds; the graphed pair steppers against the eager step, losses and fine positions bit-equal over three steps.  Inference:
the blend behind the plain pair renders.

Heads: B = 37 (a partial block), (Nc, Nf) in SHAPES: the sampler's minimum, E = 1, 2, 4, 8, a second chunk of one sample, both
size limits.  Inputs and helpers: tests/test_gpu_occupancy_graphed.py's and tests/test_gpu_occupancy_hierarchical.py's."""
import warnings

import numpy as np
import pytest
import torch

import background_model as BM
import nerf_oracle as O
import occupancy_graphed_model as G
import occupancy_hierarchical_model as H
import occupancy_model as M
import occupancy_train_model as T
import ray_routines_model as RM
import test_gpu_occupancy_graphed as OG
import test_gpu_occupancy_hierarchical as OH
from test_gpu_occupancy_graphed import ball_grid, make_net, same, tbins, to_dev_mask

pytestmark = pytest.mark.gpu

B = 37
SHAPES = ((3, 5), (64, 128), (65, 129), (16, 257), (256, 256))
COMBOS = ((False, True), (True, False), (True, True))              # (NOISE, BG): what the heads instantiate
IDS = ("Bg", "noise", "noiseBg")
MODES = ("u", "device_rng")
STD = BM.NOISE_STD
NOISE_SEED, NOISE_BASE, NOISE_OFFSET = 7, 4, 3                      # the seed directly, and as base + an offset read from device memory
RID = 77                                                            # ray id of the first ray where the jitter carries none
SENTINEL = OG.SENTINEL
_cases = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def ray_subset(oracle, synthetic):
    """B rows of the full view: 30 rays that pass the centre of the radius-1 ball within 0.8 (a chord of at least 1.2: several live
    samples from Nc = 16 on) and 7 that stay 1.2 away from it (no live sample), each spread evenly over its set"""
    if "subset" not in _cases:
        rays = OG.full_rays(oracle, synthetic).double()
        o, d = rays[:, :3], rays[:, 3:] / rays[:, 3:].norm(dim=1, keepdim=True)
        closest = (o - (o * d).sum(1, keepdim=True) * d).norm(dim=1).numpy()
        hit, miss = np.nonzero(closest < 0.8)[0], np.nonzero(closest > 1.2)[0]
        pick = lambda rows, n: rows[np.linspace(0, len(rows) - 1, n).astype(np.int64)]      # noqa: E731
        _cases["subset"] = np.sort(np.concatenate([pick(hit, B - 7), pick(miss, 7)]))
        assert len(set(_cases["subset"].tolist())) == B
    return _cases["subset"]


def case(dev, oracle, synthetic, mode, Nc, Nf):
    """One batch of a shape: rays, targets, backgrounds, the coarse jitter arguments (chain's / heads'), the sampler's, dense
    raw [B, Nc, 4] whose last sample is empty on most rays (the compositor's last delta is 1e10: acc < 1 needs that), the ball
    grid's mark under the "empty" policy and its live rows -- formed once, shared by the tests, never written to."""
    from nerf_simple_amd import _lib
    key = (mode, Nc, Nf)
    if key not in _cases:
        gen = torch.Generator().manual_seed(1000 * Nc + Nf)
        idx = torch.from_numpy(ray_subset(oracle, synthetic)).to(dev)
        rays = OG.full_rays(oracle, synthetic).to(dev)[idx].contiguous()
        u = OG.full_u(Nc).to(dev)[idx].contiguous()
        u_f = OH.full_u(Nf, salt=1).to(dev)[idx].contiguous()
        kw, ref_args, new_args, sampler = OH.jitter_args(mode, rays, u, Nc, dev)
        if mode != "device_rng":                              # the jitter carries no ray ids: the noise gets some of its own
            ref_args, new_args = ref_args[:4] + (RID,), new_args[:4] + (RID,)
        raw = torch.randn(B, Nc, 4, generator=gen)
        raw[..., 3] = 2.0 * raw[..., 3] - 1.0
        raw[torch.arange(B) % 3 != 0, -1, 3] = -40.0
        live = OG.model_live(rays, ref_args, Nc, "empty")
        m = ball_grid(dev, "empty").mark(rays, Nc, **kw)
        assert m.live == int(live.sum()), key
        ts_c = OG.query_points(rays, *ref_args, Nc)[1].contiguous()
        _cases[key] = dict(rays=rays, u_f=u_f, gt=torch.rand(B, 3, generator=gen).to(dev), bg1=torch.rand(3, generator=gen).to(dev),
                           bgB=torch.rand(B, 3, generator=gen).to(dev), ref_args=ref_args, new_args=new_args, sampler=sampler,
                           raw=raw.to(dev), live=live, m=m, total=int(live.sum()), raw_live=raw.to(dev)[torch.from_numpy(live).to(dev)],
                           ts_c=ts_c, rid=ref_args[4], uf_new=None if sampler[0] else u_f,
                           ts_args=(ts_c, None, _lib.FLAG_TS_GIVEN, 0, ref_args[4]))
    return _cases[key]


def terms_of(combo, c, k=0):
    """(bg, std) of a combination; the background alternates between one colour and one per ray with ``k``"""
    noise, bg = combo
    return (c["bg1"] if k % 2 else c["bgB"]) if bg else None, STD if noise else 0.0


def stride_of(bg):
    return 0 if bg is None or bg.dim() == 1 else 3


# ---- the entry points through ctypes -------------------------------------------------------------------------------------------
def sample_pdf(dev, ts_c, w, u_f, sampler, Nc, Nf):
    return OH.reference_sampler(ts_c, w, u_f, sampler, ts_c.shape[0], Nc, Nf, dev)


def dense_chain(dev, c, bg, std, Nc, Nf):
    """The dense coarse head's definition, stage by stage -> (rgb_bg, d_raw, ts_f, w, the noisy raw)"""
    from nerf_simple_amd import _lib
    lib, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    raw, ts, rays, gt = c["raw"], c["ts_c"], c["rays"], c["gt"]
    raw_n = raw
    if std:                                                                                                  # 1
        raw_n = torch.full_like(raw, float("nan"))
        _lib.check(lib.nerf_amd_sigma_noise(ptr(raw), ptr(raw_n), std, 0, NOISE_SEED, None, c["rid"], B, Nc, st), "noise")
    rgb, disp, acc = torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)
    w = torch.full((B, Nc), float("nan"), device=dev)
    _lib.check(lib.nerf_amd_volume_render_rays(ptr(raw_n), ptr(ts), ptr(rays), ptr(rgb), ptr(disp), None, ptr(acc), ptr(w), B, Nc, st),
               "compositor")                                                                                 # 2
    rgb_bg, g_acc = rgb, None
    if bg is not None:                                                                                       # 3
        rgb_bg = torch.empty(B, 3, device=dev)
        _lib.check(lib.nerf_amd_background_blend(ptr(rgb), ptr(acc), None, ptr(bg), stride_of(bg), ptr(rgb_bg), None, B, st), "blend")
    g = BM.mse_gradient(rgb_bg, gt).contiguous()                                                             # 4
    if bg is not None:                                                                                       # 5
        g_acc = torch.empty(B, device=dev)
        _lib.check(lib.nerf_amd_background_blend_backward(ptr(g), ptr(bg), stride_of(bg), ptr(g_acc), B, st), "blend backward")
    d = torch.full((B, Nc, 4), float("nan"), device=dev)
    _lib.check(lib.nerf_amd_volume_render_rays_backward(ptr(raw_n), ptr(ts), ptr(rays), ptr(g), None, None, ptr(g_acc), None, ptr(d),
                                                        B, Nc, st), "compositor backward")                  # 6
    return rgb_bg, d, sample_pdf(dev, ts, w, c["u_f"], c["sampler"], Nc, Nf), w, raw_n                       # 7


def dense_head(dev, c, bg, std, Nc, Nf, pad=8):
    """-> (rgb, d_raw, the sentinel-prefilled flat ts_out buffer); the noise seed comes as NOISE_BASE + an offset of NOISE_OFFSET
    read from device memory, the sampler's seed (device_rng) likewise: as a graph node takes them"""
    from nerf_simple_amd import _lib
    jit, _, flags, seed, rid = c["new_args"]
    off = torch.tensor([NOISE_OFFSET], dtype=torch.int64, device=dev)
    rgb = torch.full((B, 3), SENTINEL, device=dev)
    d = torch.full((B, Nc, 4), SENTINEL, device=dev)
    ts_out = torch.full((B * (Nc + Nf) + pad,), SENTINEL, device=dev)
    u = jit if flags & _lib.FLAG_SEED_IN_MEMORY else c["uf_new"]
    _lib.check(_lib.lib().nerf_amd_volume_render_mse_backward_pdf_bg(
        _lib.ptr(c["raw"]), _lib.ptr(c["ts_c"]), _lib.ptr(c["rays"]), _lib.ptr(c["gt"]), _lib.ptr(bg), stride_of(bg), std,
        _lib.FLAG_SEED_IN_MEMORY, NOISE_BASE, _lib.ptr(off), _lib.ptr(u), flags, seed, rid, _lib.ptr(rgb), _lib.ptr(d),
        _lib.ptr(ts_out), B, Nc, Nf, _lib.stream_ptr(dev)), "dense coarse head")
    return rgb, d, ts_out


def masked_chain(dev, c, raw_kept, args, mask_c, offsets_c, bg, std, Nc, Nf):
    """The masked coarse head's definition under mask_C / offsets_C -> (rgb_bg, d_raw of the kept rows, ts_f, w, noisy rows)"""
    from nerf_simple_amd import _lib
    lib, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    jit, tb, flags, seed, rid = args
    rays, gt = c["rays"], c["gt"]
    K = raw_kept.shape[0]
    raw_n = raw_kept
    if std and K:                                                                                            # 1
        raw_n = torch.full_like(raw_kept, float("nan"))
        _lib.check(lib.nerf_amd_sigma_noise_masked(ptr(raw_kept), ptr(raw_n), std, 0, NOISE_SEED, None, rid, ptr(mask_c), ptr(offsets_c),
                                                   B, Nc, st), "masked noise")
    rgb, disp, acc = torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)
    w = torch.full((B, Nc), float("nan"), device=dev)
    hd = (ptr(raw_n) if K else None, ptr(rays), ptr(jit), ptr(tb), flags, seed, rid, ptr(mask_c), ptr(offsets_c))
    _lib.check(lib.nerf_amd_volume_render_masked(*hd, ptr(rgb), ptr(disp), None, ptr(acc), ptr(w), B, Nc, st), "masked compositor")  # 2
    rgb_bg, g_acc = rgb, None
    if bg is not None:                                                                                       # 3
        rgb_bg = torch.empty(B, 3, device=dev)
        _lib.check(lib.nerf_amd_background_blend(ptr(rgb), ptr(acc), None, ptr(bg), stride_of(bg), ptr(rgb_bg), None, B, st), "blend")
    g = BM.mse_gradient(rgb_bg, gt).contiguous()                                                             # 4
    if bg is not None:                                                                                       # 5
        g_acc = torch.empty(B, device=dev)
        _lib.check(lib.nerf_amd_background_blend_backward(ptr(g), ptr(bg), stride_of(bg), ptr(g_acc), B, st), "blend backward")
    d = torch.full((K, 4), float("nan"), device=dev)
    _lib.check(lib.nerf_amd_volume_render_masked_backward(*hd, ptr(g), None, None, ptr(g_acc), None, ptr(d) if K else None, B, Nc, st),
               "masked backward")                                                                            # 6
    return rgb_bg, d, sample_pdf(dev, c["ts_c"], w, c["u_f"], c["sampler"], Nc, Nf), w, raw_n                # 7


def masked_head(dev, c, raw, args, mask, offsets, bg, std, C, Nc, Nf, pad=8):
    """-> (rgb, the whole sentinel-prefilled d_raw buffer [C + pad, 4], the sentinel-prefilled flat ts_out buffer)"""
    from nerf_simple_amd import _lib
    jit, tb, flags, seed, rid = args
    off = torch.tensor([NOISE_OFFSET], dtype=torch.int64, device=dev)
    rgb = torch.full((B, 3), SENTINEL, device=dev)
    buf = torch.full((C + pad, 4), SENTINEL, device=dev)
    ts_out = torch.full((B * (Nc + Nf) + pad,), SENTINEL, device=dev)
    _lib.check(_lib.lib().nerf_amd_volume_render_masked_mse_backward_pdf_bg(
        _lib.ptr(raw), _lib.ptr(c["rays"]), _lib.ptr(jit), _lib.ptr(tb), flags, seed, rid, _lib.ptr(mask), _lib.ptr(offsets),
        _lib.ptr(c["gt"]), _lib.ptr(bg), stride_of(bg), std, _lib.FLAG_SEED_IN_MEMORY, NOISE_BASE, _lib.ptr(off), _lib.ptr(c["uf_new"]),
        _lib.ptr(rgb), _lib.ptr(buf), _lib.ptr(ts_out), C, B, Nc, Nf, _lib.stream_ptr(dev)), "masked coarse head")
    return rgb, buf, ts_out


def capacities(live, total):
    """exactly P', surplus rows, and an overflow that cuts inside a ray (between two rays where no ray holds two live samples)"""
    starts = set(M.offsets(live).tolist())
    cut = next((C for C in range(-(-total // 2), total) if C not in starts), -(-total // 2))
    return total, total + 5, cut


# ---- 1. the inputs ---------------------------------------------------------------------------------------------------------------
def test_the_batches_are_informative(dev, oracle, synthetic):
    """By the CPU oracle: the blend matters (a quarter of the rays keep acc < 0.99), the noise moves the sampler (ts_f changes on
    half of the rays), and the masked cases hold live rays, dead rays and rays the overflowing capacity cuts."""
    cut_inside = 0
    for Nc, Nf in SHAPES:
        c = case(dev, oracle, synthetic, "u", Nc, Nf)
        rays, ts_c, u_f, live = c["rays"].cpu(), c["ts_c"].cpu(), c["u_f"].cpu(), c["live"]
        dn = BM.unit_dirs(rays)
        z, _ = BM.noise_normal(NOISE_SEED, RID, B, Nc)
        dense = c["raw"].cpu()
        masked = T.scatter_live(c["raw_live"].cpu(), live)
        for what, raw in (("dense", dense), ("masked", masked)):
            noisy = raw.clone()
            noisy[..., 3] = (raw[..., 3].double() + STD * torch.from_numpy(z)).float()        # -inf stays -inf
            plain, out = O.volume_render(raw, ts_c, dn), O.volume_render(noisy, ts_c, dn)
            assert int((out[3] < 0.99).sum()) >= B / 4 and int((plain[3] < 0.99).sum()) >= B / 4, (what, Nc, Nf)
            moved = (O.sample_pdf(ts_c, plain[4], u_f) != O.sample_pdf(ts_c, out[4], u_f)).any(1)
            print(f"{what} ({Nc}, {Nf}): acc < 0.99 on {int((out[3] < 0.99).sum())} of {B} rays, the noise moves ts_f on {int(moved.sum())}")
            # Nc = 3 leaves the sampler ONE interior bin: its placement cannot depend on the weights
            assert int(moved.sum()) >= B / 2 or Nc == 3, (what, Nc, Nf, int(moved.sum()))
        n = live.sum(1)
        kept = G.mask_C(live, capacities(live, c["total"])[2]).sum(1)
        assert (n == 0).any() and (n > 0).any() and (kept < n).any(), (Nc, Nf)
        assert ((kept > 0) & (kept < n)).any() or n.max() < 2, (Nc, Nf)           # cut inside a ray wherever a ray can be cut
        cut_inside += int(((kept > 0) & (kept < n)).any())
    assert cut_inside >= len(SHAPES) - 1


# ---- 2. the dense coarse head is its chain ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("combo", COMBOS, ids=IDS)
def test_dense_head_is_the_chain(dev, oracle, synthetic, combo, mode):
    for k, (Nc, Nf) in enumerate(SHAPES):
        c = case(dev, oracle, synthetic, mode, Nc, Nf)
        bg, std = terms_of(combo, c, k)
        where = (combo, mode, Nc, Nf)
        rgb_ref, d_ref, ts_ref, _, _ = dense_chain(dev, c, bg, std, Nc, Nf)
        rgb, d, tbuf = dense_head(dev, c, bg, std, Nc, Nf)
        rgb2, d2, tbuf2 = dense_head(dev, c, bg, std, Nc, Nf)
        assert same(rgb, rgb2) and same(d, d2) and same(tbuf, tbuf2), where                    # two runs, the same bytes
        assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(tbuf[:B * (Nc + Nf)]).all()), where
        assert same(rgb, rgb_ref), where
        assert same(d, d_ref), where
        assert same(tbuf[:B * (Nc + Nf)].view(B, Nc + Nf), ts_ref), where
        assert bool((tbuf[B * (Nc + Nf):] == SENTINEL).all()), where                          # nothing beyond ts_out
        if combo[0] and Nc > 3:                                                               # the sampler saw the noisy weights
            assert not same(ts_ref, dense_chain(dev, c, bg, 0.0, Nc, Nf)[2]), where


@pytest.mark.parametrize("mode", MODES)
def test_dense_head_with_no_term_is_the_plain_coarse_head(dev, oracle, synthetic, mode):
    from nerf_simple_amd import _lib
    for Nc, Nf in SHAPES:
        c = case(dev, oracle, synthetic, mode, Nc, Nf)
        rgb, d, tbuf = dense_head(dev, c, None, 0.0, Nc, Nf)
        jit, _, flags, seed, rid = c["new_args"]
        rgb_p, d_p = torch.full_like(rgb, SENTINEL), torch.full_like(d, SENTINEL)
        t_p = torch.full_like(tbuf, SENTINEL)
        u = jit if flags & _lib.FLAG_SEED_IN_MEMORY else c["uf_new"]
        _lib.check(_lib.lib().nerf_amd_volume_render_mse_backward_pdf(
            _lib.ptr(c["raw"]), _lib.ptr(c["ts_c"]), _lib.ptr(c["rays"]), _lib.ptr(c["gt"]), _lib.ptr(u), flags, seed, rid,
            _lib.ptr(rgb_p), _lib.ptr(d_p), _lib.ptr(t_p), B, Nc, Nf, _lib.stream_ptr(dev)), "plain coarse head")
        assert same(rgb, rgb_p) and same(d, d_p) and same(tbuf, t_p), (mode, Nc, Nf)


# ---- 3. the masked coarse head is its chain under mask C -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("combo", COMBOS, ids=IDS)
def test_masked_head_is_the_chain_under_mask_C(dev, oracle, synthetic, combo, mode):
    for Nc, Nf in SHAPES:
        c = case(dev, oracle, synthetic, mode, Nc, Nf)
        live, total, m, raw_live = c["live"], c["total"], c["m"], c["raw_live"]
        for k, C in enumerate(capacities(live, total)):
            where = (combo, mode, Nc, Nf, C, total)
            bg, std = terms_of(combo, c, k)
            kept = min(total, C)
            kept_mask = G.mask_C(live, C)
            mask_c, offsets_c = to_dev_mask(kept_mask, dev)
            raw = torch.full((C, 4), float("nan"), device=dev)                    # rows beyond `kept`: NaN, never read
            raw[:kept] = raw_live[:kept]
            rgb_ref, d_ref, ts_ref, w_ref, _ = masked_chain(dev, c, raw_live[:kept].contiguous(), c["ref_args"], mask_c, offsets_c, bg, std,
                                                            Nc, Nf)
            rgb, dbuf, tbuf = masked_head(dev, c, raw, c["new_args"], m.mask, m.offsets, bg, std, C, Nc, Nf)
            rgb2, dbuf2, tbuf2 = masked_head(dev, c, raw, c["new_args"], m.mask, m.offsets, bg, std, C, Nc, Nf)
            assert same(rgb, rgb2) and same(dbuf, dbuf2) and same(tbuf, tbuf2), where          # two runs, the same bytes
            assert same(rgb, rgb_ref), where
            ts_out = tbuf[:B * (Nc + Nf)].view(B, Nc + Nf)
            assert same(ts_out, ts_ref) and bool(torch.isfinite(ts_out).all()), where
            assert bool((tbuf[B * (Nc + Nf):] == SENTINEL).all()), where
            assert bool((dbuf[kept:C] == 0).all()) and bool((dbuf[C:] == SENTINEL).all()), where   # surplus rows; nothing beyond C
            assert bool(torch.isfinite(d_ref).all()) and same(dbuf[:kept], d_ref), where
            assert not bool(w_ref[torch.from_numpy(~kept_mask).to(dev)].any()), where              # exactly 0 at a dead sample
            # a ray with nothing kept: rgb = bg exactly, and the sampler's uniform rows
            none = torch.from_numpy(kept_mask.sum(1) == 0).to(dev)
            want_bg = torch.zeros(B, 3, device=dev) if bg is None else bg.expand(B, 3)
            assert same(rgb[none], want_bg[none]), where
            zero = sample_pdf(dev, c["ts_c"], torch.zeros_like(w_ref), c["u_f"], c["sampler"], Nc, Nf)
            assert same(ts_out[none], zero[none]), where


@pytest.mark.parametrize("combo", COMBOS, ids=IDS)
def test_all_live_grid_is_the_dense_head(dev, oracle, synthetic, combo):
    for k, (Nc, Nf) in enumerate(SHAPES):
        for mode in MODES:
            c = case(dev, oracle, synthetic, mode, Nc, Nf)
            bg, std = terms_of(combo, c, k)
            mask, offsets = to_dev_mask(np.ones((B, Nc), bool), dev)
            # given uniforms: the walk reads the dense head's own positions; the counter RNG: the sampler's seed is the jitter's
            args = c["new_args"] if mode == "device_rng" else c["ts_args"]
            rgb, dbuf, tbuf = masked_head(dev, c, c["raw"].view(-1, 4), args, mask, offsets, bg, std, B * Nc, Nc, Nf)
            rgb_d, d_d, t_d = dense_head(dev, c, bg, std, Nc, Nf)
            assert same(rgb, rgb_d) and same(dbuf[:B * Nc], d_d.view(-1, 4)) and same(tbuf, t_d), (combo, mode, Nc, Nf)
            assert bool((dbuf[B * Nc:] == SENTINEL).all())


@pytest.mark.parametrize("combo", COMBOS, ids=IDS)
def test_all_dead_batch(dev, oracle, synthetic, combo):
    """nothing live: rgb = bg exactly (0 without one), every row of d_raw_live a zero, the sampler's uniform placement"""
    for k, (Nc, Nf) in enumerate(SHAPES):
        c = case(dev, oracle, synthetic, "u", Nc, Nf)
        bg, std = terms_of(combo, c, k)
        mask, offsets = to_dev_mask(np.zeros((B, Nc), bool), dev)
        C = 11
        raw = torch.full((C, 4), float("nan"), device=dev)
        rgb, dbuf, tbuf = masked_head(dev, c, raw, c["new_args"], mask, offsets, bg, std, C, Nc, Nf)
        assert same(rgb, torch.zeros(B, 3, device=dev) if bg is None else bg.expand(B, 3).contiguous()), (combo, Nc, Nf)
        assert bool((dbuf[:C] == 0).all()) and bool((dbuf[C:] == SENTINEL).all()), (combo, Nc, Nf)
        ts_out = tbuf[:B * (Nc + Nf)].view(B, Nc + Nf)
        zero = sample_pdf(dev, c["ts_c"], torch.zeros(B, Nc, device=dev), c["u_f"], c["sampler"], Nc, Nf)
        assert same(ts_out, zero), (combo, Nc, Nf)
        # ... which is the oracle's uniform_rows to the sampler's own accuracy on these positions (a few ulps of tf = 6)
        want = H.uniform_rows(c["ts_c"].cpu().double(), c["u_f"].cpu().double())
        assert float((ts_out.cpu().double() - want).abs().max()) <= 64 * BM.EPS * 6.0, (combo, Nc, Nf)


# ---- 4. a dead sample stays dead -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_dead_sample_stays_dead_whatever_the_noise(dev, oracle, synthetic, mode):
    for Nc, Nf in SHAPES:
        c = case(dev, oracle, synthetic, mode, Nc, Nf)
        live, total, m = c["live"], c["total"], c["m"]
        for C in capacities(live, total)[::2]:                                     # exactly P', and the overflow inside a ray
            kept = min(total, C)
            kept_mask = G.mask_C(live, C)
            mask_c, offsets_c = to_dev_mask(kept_mask, dev)
            raw = torch.full((C, 4), float("nan"), device=dev)
            raw[:kept] = c["raw_live"][:kept]
            rgb, dbuf, tbuf = masked_head(dev, c, raw, c["new_args"], m.mask, m.offsets, c["bgB"], 1e30, C, Nc, Nf)
            ts_out = tbuf[:B * (Nc + Nf)].view(B, Nc + Nf)
            assert bool(torch.isfinite(ts_out).all()) and bool(torch.isfinite(dbuf[:C]).all()) and bool(torch.isfinite(rgb).all())
            _, _, ts_ref, w_ref, _ = masked_chain(dev, c, c["raw_live"][:kept].contiguous(), c["ref_args"], mask_c, offsets_c, c["bgB"],
                                                  1e30, Nc, Nf)
            dead = torch.from_numpy(~kept_mask).to(dev)
            assert not bool(w_ref[dead].any()) and not bool(torch.isnan(w_ref).any()), (mode, Nc, Nf, C)
            assert same(ts_out, ts_ref), (mode, Nc, Nf, C)


# ---- 5. float64 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["dense", "masked"])
def test_head_against_float64(dev, oracle, synthetic, which):
    """d_raw of the head with both terms against the float64 gradient of MSE(rgb + (1 - acc) bg, gt) on the noisy raw (the noise
    read back from the stage; the masked rows scattered into a dense raw with (0, 0, 0, -inf) at the dead samples): the compositor
    backward's per-ray rule with the constants of tests/background_model.py, as tests/test_gpu_background.py and
    tests/test_gpu_masked_controls.py apply it."""
    Nc, Nf = (65, 129) if which == "dense" else (64, 128)
    c = case(dev, oracle, synthetic, "u", Nc, Nf)
    bg = c["bgB"]
    if which == "dense":
        _, _, _, _, raw_n = dense_chain(dev, c, bg, STD, Nc, Nf)
        rgb_h, d_h, _ = dense_head(dev, c, bg, STD, Nc, Nf)
        noisy, live, got = raw_n.cpu(), np.ones((B, Nc), bool), d_h.cpu().double().numpy()
    else:
        live, total, m = c["live"], c["total"], c["m"]
        _, _, _, _, rows = masked_chain(dev, c, c["raw_live"], c["ref_args"], m.mask, m.offsets, bg, STD, Nc, Nf)
        rgb_h, dbuf, _ = masked_head(dev, c, c["raw_live"], c["new_args"], m.mask, m.offsets, bg, STD, total, Nc, Nf)
        noisy = T.scatter_live(rows.cpu(), live)
        got = np.zeros((B, Nc, 4))
        got[live] = dbuf[:total].cpu().double().numpy()
    cpu = (noisy, c["ts_c"].cpu(), c["rays"].cpu(), c["gt"].cpu(), bg.cpu())
    want, A, rgb64 = BM.head_model(*cpu)
    keep = np.isfinite(BM.oracle_head_grad(*cpu, torch.float32)) & live[:, :, None]
    assert np.isfinite(got[keep]).all()
    assert np.abs(rgb_h.cpu().double().numpy() - rgb64).max() <= 64 * BM.EPS * max(1.0, np.abs(rgb64).max())
    cond, plain = RM.ray_ratios(got, want, A, keep)
    r_cond, r_plain = float(cond.max()), float(np.nanmax(plain, initial=0.0))
    print(f"{which} coarse head vs float64: conditioned {r_cond:.2f} of {RM.bound(BM.C_REF_BG):.1f}, plain {r_plain:.2f} of "
          f"{RM.bound(BM.C_REF_BG_PLAIN):.1f}")
    assert r_cond <= RM.bound(BM.C_REF_BG) and r_plain <= RM.bound(BM.C_REF_BG_PLAIN)


# ---- 6. the eager step -----------------------------------------------------------------------------------------------------------
def pair_of(dev, kind="default", precision="bf16"):
    return make_net(dev, kind, precision), OH.make_net(dev, kind, precision, seed=1)


def by_hand(dev, nets, occ, rays, gt, u_c, u_f, Nc, Nf, controls, rid, fine_offset):
    """[MSE(blend(coarse)), MSE(blend(fine))] and ts_f from the public renders under the two noise seeds; the blend as torch's own
    fp32 expression (two rounded operations per channel, the kernel's)"""
    from nerf_simple_amd import training
    from nerf_simple_amd.utils import rendering
    Controls = training.Controls
    bg = controls.background
    cc = Controls(sigma_noise=controls.sigma_noise, noise_seed=controls.noise_seed)
    cf = cc.replace(noise_seed=(controls.noise_seed + fine_offset) % (1 << 64))
    kw_c, kw_f = ({"controls": cc}, {"controls": cf}) if controls.sigma_noise else ({}, {})
    if occ is None:
        coarse = rendering.render_nerf(rays, nets[0], Nc, u=u_c, ray_id0=rid, **kw_c)
        ts_c = OG.query_points(rays, u_c, tbins(Nc, dev), 0, 0, 0, Nc)[1]
    else:
        coarse, ts_c = training.render_nerf_masked(rays, nets[0], Nc, occ, u=u_c, ray_id0=rid, return_ts=True, **kw_c)
    ts_f = rendering.sample_pdf(ts_c, coarse[4].detach(), Nf, u=u_f)
    if occ is None:
        fine = rendering.render_nerf(rays, nets[1], Nc + Nf, ts=ts_f, ray_id0=rid, **kw_f)
    else:
        fine = training.render_nerf_masked(rays, nets[1], Nc + Nf, occ, ts=ts_f, ray_id0=rid, **kw_f)
    blend = (lambda o: o[0]) if bg is None else (lambda o: o[0] + (1 - o[3])[:, None] * bg)
    return [training.mse_loss(blend(o), gt).detach() for o in (coarse, fine)], ts_f


@pytest.mark.parametrize("path", ["dense", "masked", "dense-fp32"])
def test_eager_step_is_the_torch_expression(dev, oracle, synthetic, path):
    from nerf_simple_amd import training
    Nc, Nf = (16, 24) if path == "dense-fp32" else (64, 128)
    precision = "fp32" if path == "dense-fp32" else "bf16"
    rays, gt, u_c, u_f = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, B, Nc, Nf))
    occ = ball_grid(dev, "empty") if path == "masked" else None
    bgB = torch.rand(B, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    for bg, std in ((bgB, STD), (bgB[0].contiguous(), 0.0), (None, STD)):
        c = training.Controls(background=bg, sigma_noise=std, noise_seed=21)
        nets = pair_of(dev, precision=precision)
        opt = torch.optim.SGD([p for n in nets for p in n.parameters()], lr=0.0)
        out = training.train_step_hierarchical(*nets, opt, rays, gt, Nc, Nf, u_c=u_c, u_f=u_f, ray_id0=9, occupancy=occ, controls=c)
        want, ts_f = by_hand(dev, pair_of(dev, precision=precision), occ, rays, gt, u_c, u_f, Nc, Nf, c, 9, training.FINE_NOISE_OFFSET)
        where = (path, bg is not None, std)
        assert same(out.losses[0], want[0]) and same(out.losses[1], want[1]), (where, out.losses, want)
        assert same(out.ts_f, ts_f) and same(out, out.losses[0] + out.losses[1]), where
        if std:       # one key for both passes gives another fine loss: the streams are really two
            one, _ = by_hand(dev, pair_of(dev, precision=precision), occ, rays, gt, u_c, u_f, Nc, Nf, c, 9, 0)
            assert same(one[0], want[0]) and not same(one[1], want[1]), where
    # the terms did matter
    nets = pair_of(dev, precision=precision)
    opt = torch.optim.SGD([p for n in nets for p in n.parameters()], lr=0.0)
    plain = training.train_step_hierarchical(*nets, opt, rays, gt, Nc, Nf, u_c=u_c, u_f=u_f, ray_id0=9, occupancy=occ)
    assert not same(plain.losses[0], out.losses[0]) and not same(plain.ts_f, out.ts_f)


# ---- 7. the graphed steppers -----------------------------------------------------------------------------------------------------
def eager_pair(dev, nets, occ, rays, gt, Nc, Nf, controls, **kw):
    from nerf_simple_amd import training
    opt = torch.optim.SGD([p for n in nets for p in n.parameters()], lr=0.0)
    return training.train_step_hierarchical(*nets, opt, rays, gt, Nc, Nf, occupancy=occ, controls=controls, **kw)


@pytest.mark.parametrize("shape", [(576, 64, 128), (37, 66, 65)])
def test_graphed_pair_is_the_eager_pair(dev, oracle, synthetic, shape):
    """three replays with device_rng=True against the eager step with seed + k and noise_seed + k; the background is overwritten
    in place behind replay 2"""
    from nerf_simple_amd import training
    from nerf_simple_amd.optim import FusedAdam
    Bn, Nc, Nf = shape
    rays, gt, _, _ = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, Bn, Nc, Nf))
    bg = torch.rand(Bn, 3, generator=torch.Generator().manual_seed(8)).to(dev)
    if Bn == 37:
        bg = bg[0].contiguous()
    c = training.Controls(background=bg, sigma_noise=STD, noise_seed=900)
    nets, twins = pair_of(dev, "structured"), pair_of(dev, "structured")
    stepper = training.GraphedHierarchicalTrainStep(*nets, FusedAdam(list(nets), lr=0.0), Bn, Nc, Nf, device_rng=True, seed=40,
                                                    ray_id0=11, controls=c)
    assert stepper.background.data_ptr() != bg.data_ptr() and stepper.sigma_noise == STD
    with pytest.raises(AttributeError):
        stepper.sigma_noise = 0.1
    seen = []
    for k in (1, 2, 3):
        if k == 3:
            bg = 1.0 - bg
            stepper.background.copy_(bg)                                          # in place: the next replay reads it
        total = stepper.step(rays, gt).clone()
        want = eager_pair(dev, twins, None, rays, gt, Nc, Nf, c.replace(noise_seed=c.noise_seed + k, background=bg),
                          device_rng=True, seed=40 + k, ray_id0=11)
        assert same(stepper.losses, torch.stack(want.losses)), (shape, k, stepper.losses.tolist(), [float(x) for x in want.losses])
        assert same(stepper.ts_f, want.ts_f) and same(total, want), (shape, k)
        seen.append(float(total))
    # (whether the new background CHANGES the dense loss depends on the nets: the compositor's last interval is 1e10, so a ray is
    # opaque wherever the last density is not strongly negative, and the blend is then the identity.  The masked stepper's test
    # below shows the effect of the overwrite.)
    assert len(set(seen)) == 3


def masked_pair_under_caps(dev, nets, occ, rays, gt, u_c, u_f, Nc, Nf, controls, rid, C_c):
    """the eager masked pair step with its coarse pass under mask_C(live_c, C_c): the existing autograd functions composed by
    hand (tests/test_gpu_occupancy_hierarchical.py::eager_step with the noise stage and the blend) -> ([loss_c, loss_f], ts_f)"""
    from nerf_simple_amd import training
    from nerf_simple_amd.utils.rendering import sample_pdf as sampler
    Bn = rays.shape[0]
    bg, stride = (controls.background, 0) if controls.background.dim() == 1 else (controls.background, 3)
    m = occ.mark(rays, Nc, points=True, u=u_c)
    kept_mask = G.mask_C(OH.M_unpack(m.mask, Nc), C_c)
    K = int(kept_mask.sum())
    mask_c, offsets_c = to_dev_mask(kept_mask, dev)
    params = [p for _, p in nets[0].named_parameters()]
    raw, _ = training._FusedDense.apply(nets[0], None, None, None, 0, 0, 0, 1, m.points[:K].contiguous(), *params)
    raw = training._MaskedSigmaNoise.apply(raw.reshape(-1, 4), controls.sigma_noise, controls.noise_seed, rid, (mask_c, offsets_c, Bn, Nc))
    outs = training._MaskedVolumeRender.apply(raw, (rays, u_c, tbins(Nc, dev), 0, 0, 0, mask_c, offsets_c), Bn, Nc)
    loss_c = training.mse_loss(training._Background.apply(outs[0], outs[3], bg.contiguous(), stride), gt)
    loss_c.backward()
    ts_c = OG.query_points(rays, u_c, tbins(Nc, dev), 0, 0, 0, Nc)[1]
    ts_f = sampler(ts_c, outs[4].detach(), Nf, u=u_f)
    fine = training.render_nerf_masked(rays, nets[1], Nc + Nf, occ, ts=ts_f, ray_id0=rid,
                                       controls=controls.replace(noise_seed=(controls.noise_seed + training.FINE_NOISE_OFFSET) % (1 << 64)))
    loss_f = training.mse_loss(fine[0], gt)
    loss_f.backward()
    return torch.stack([loss_c.detach(), loss_f.detach()]), ts_f


@pytest.mark.parametrize("case_", [(576, 64, 128), (37, 66, 65)])
def test_graphed_masked_pair_is_the_eager_masked_pair(dev, oracle, synthetic, case_):
    """given u_c / u_f, three replays: at tight capacities (the eager steps' own live counts, their maximum over the three steps)
    against the eager masked pair step; with a coarse capacity that cuts inside a ray against the eager composition under mask_C"""
    from nerf_simple_amd import training
    from nerf_simple_amd.optim import FusedAdam
    Bn, Nc, Nf = case_
    rays, gt, u_c, u_f = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, Bn, Nc, Nf))
    occ = ball_grid(dev, "empty")
    bg = torch.rand(Bn, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    if Bn == 37:
        bg = bg[0].contiguous()
    c = training.Controls(background=bg, sigma_noise=STD, noise_seed=300)
    twins = pair_of(dev)
    wants, counts = [], []
    for k in (1, 2, 3):                  # the background is overwritten in place behind replay 2
        wants.append(eager_pair(dev, twins, occ, rays, gt, Nc, Nf, c.replace(noise_seed=c.noise_seed + k, background=bg if k < 3 else 1.0 - bg),
                                u_c=u_c, u_f=u_f, ray_id0=5))
        counts.append((occ.last_stats["coarse"]["live"], occ.last_stats["fine"]["live"]))
    old_bg = eager_pair(dev, twins, occ, rays, gt, Nc, Nf, c.replace(noise_seed=c.noise_seed + 3), u_c=u_c, u_f=u_f, ray_id0=5)
    assert not same(old_bg.losses[0], wants[2].losses[0]) and not same(old_bg.losses[1], wants[2].losses[1])    # it does matter
    assert same(old_bg.ts_f, wants[2].ts_f)                                        # ... and never touches the sampler's weights
    Pc = counts[0][0]
    assert all(n == Pc for n, _ in counts) and 0 < Pc < Bn * Nc                     # the coarse count follows the jitter alone
    tight = (Pc, max(f for _, f in counts))
    nets = pair_of(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                             # an overflow report would raise
        stepper = training.GraphedMaskedHierarchicalTrainStep(*nets, FusedAdam(list(nets), lr=0.0), Bn, Nc, Nf, occ, tight, ray_id0=5,
                                                              controls=c)
        assert stepper.background.data_ptr() != bg.data_ptr() and stepper.sigma_noise == STD
        for k in (1, 2, 3):
            if k == 3:
                stepper.background.copy_(1.0 - bg)                                 # in place: the next replay reads it
            total = stepper.step(rays, gt, u_c=u_c, u_f=u_f).clone()
            want = wants[k - 1]
            assert same(stepper.losses, torch.stack(want.losses)), (case_, k, stepper.losses.tolist(), [float(x) for x in want.losses])
            assert same(stepper.ts_f, want.ts_f) and same(total, want), (case_, k)
            now = stepper.counts()
            assert (now["coarse"]["live"], now["fine"]["live"]) == counts[k - 1] and now["fine"]["kept"] == counts[k - 1][1]
    assert not same(wants[0].ts_f, wants[1].ts_f)                                  # the noise moved the sampler from step to step
    # an overflowing coarse capacity: the sampler sees the noisy weights under the stricter mask
    live_c = OG.model_live(rays, (u_c, tbins(Nc, dev), 0, 0, 0), Nc, "empty")
    C_c = capacities(live_c, Pc)[2]
    nets, twins = pair_of(dev), pair_of(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        stepper = training.GraphedMaskedHierarchicalTrainStep(*nets, FusedAdam(list(nets), lr=0.0), Bn, Nc, Nf, occ, (C_c, 1.0), ray_id0=5,
                                                              controls=c)
        for k in (1, 2, 3):
            stepper.step(rays, gt, u_c=u_c, u_f=u_f)
            for net in twins:
                net.zero_grad(set_to_none=True)
            losses, ts_f = masked_pair_under_caps(dev, twins, occ, rays, gt, u_c, u_f, Nc, Nf, c.replace(noise_seed=c.noise_seed + k), 5, C_c)
            assert same(stepper.losses, losses), (case_, k, "overflow", stepper.losses.tolist(), losses.tolist())
            assert same(stepper.ts_f, ts_f) and not same(ts_f, wants[k - 1].ts_f), (case_, k)
        assert stepper.counts()["coarse"] == {"samples": Bn * Nc, "live": Pc, "kept": C_c, "capacity": C_c}


def captured_launches(monkeypatch, build):
    """the names training._launch saw while ``build`` constructed (warmed up and captured) a stepper"""
    from nerf_simple_amd import training
    names, real = [], training._launch

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(training, "_launch", spy)
    build()
    monkeypatch.setattr(training, "_launch", real)
    return names


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "masked"])
def test_the_launch_list_is_the_plain_pairs_but_for_the_two_heads(monkeypatch, dev, masked):
    from nerf_simple_amd import training
    from nerf_simple_amd.optim import FusedAdam
    Bn, Nc, Nf = 37, 66, 65
    c = training.Controls(background=(1.0, 0.5, 0.25), sigma_noise=STD, noise_seed=1)

    def build(**kw):
        nets = pair_of(dev)
        opt = FusedAdam(list(nets), lr=0.0)
        if masked:
            return training.GraphedMaskedHierarchicalTrainStep(*nets, opt, Bn, Nc, Nf, ball_grid(dev, "empty"), (0.5, 0.5), **kw)
        return training.GraphedHierarchicalTrainStep(*nets, opt, Bn, Nc, Nf, **kw)

    plain = captured_launches(monkeypatch, build)
    empty = captured_launches(monkeypatch, lambda: build(controls=training.Controls()))
    with_c = captured_launches(monkeypatch, lambda: build(controls=c))
    assert empty == plain and len(with_c) == len(plain) and len(plain) > 0
    changed = {(a, b) for a, b in zip(plain, with_c) if a != b}
    if masked:
        assert changed == {("nerf_amd_volume_render_masked_mse_backward_pdf", "nerf_amd_volume_render_masked_mse_backward_pdf_bg"),
                           ("nerf_amd_volume_render_masked_mse_backward", "nerf_amd_volume_render_masked_mse_backward_dist")}, changed
    else:
        assert changed == {("nerf_amd_volume_render_mse_backward_pdf", "nerf_amd_volume_render_mse_backward_pdf_bg"),
                           ("nerf_amd_volume_render_mse_backward", "nerf_amd_volume_render_mse_backward_bg")}, changed


# ---- 8. inference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["dense", "masked"])
def test_inference_renders_blend_behind_the_pair(dev, oracle, synthetic, masked):
    from nerf_simple_amd.training import Controls
    from nerf_simple_amd.utils import metrics
    from nerf_simple_amd.utils.rendering import generate_rays, render_hierarchical, render_hierarchical_view
    Nc, Nf = 64, 128
    rays, _, u_c, u_f = (x.to(dev) for x in H.pair_inputs(oracle, synthetic, B, Nc, Nf))
    nets = pair_of(dev, "structured")
    kw = {"occupancy": ball_grid(dev, "empty")} if masked else {}
    bgB = torch.rand(B, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    with torch.no_grad():
        plain = render_hierarchical(rays, *nets, Nc, Nf, u_c=u_c, u_f=u_f, **kw)
        for bg in (bgB, bgB[0].contiguous()):
            got = render_hierarchical(rays, *nets, Nc, Nf, u_c=u_c, u_f=u_f, controls=Controls(background=bg), **kw)
            assert same(got[2], plain[2])                                          # ts_fine
            for g, p in zip(got[:2], plain[:2]):                                   # the fine and the coarse 5-tuple
                assert same(g[0], p[0] + (1 - p[3])[:, None] * bg) and not same(g[0], p[0])
                assert all(same(a, b) for a, b in zip(g[1:], p[1:]))
        # a view: the clip behind the blend
        pose = torch.from_numpy(np.asarray(oracle.spherical_to_pose(4, 30, 45))).float()
        cam = [8, 8, synthetic.focal_from_fov(8)]
        vu_c = torch.rand(64, Nc, generator=torch.Generator().manual_seed(1)).to(dev)
        vu_f = torch.rand(64, Nf, generator=torch.Generator().manual_seed(2)).to(dev)
        bg = torch.tensor([1.0, 0.5, 0.0], device=dev)
        fine = render_hierarchical(generate_rays(pose, cam, dev), *nets, Nc, Nf, u_c=vu_c, u_f=vu_f, **kw)[0]
        px = render_hierarchical_view(*nets, pose, cam, Nc, Nf, u_c=vu_c, u_f=vu_f, controls=Controls(background=bg), **kw)
        assert same(px[:, :3], torch.clip(fine[0] + (1 - fine[3])[:, None] * bg, 0., 1.)) and same(px[:, 3], fine[1])
        assert not same(px, render_hierarchical_view(*nets, pose, cam, Nc, Nf, u_c=vu_c, u_f=vu_f, **kw))
        # evaluate() needs nothing new: its render is a callable
        import types
        table = torch.rand(64, 3, generator=torch.Generator().manual_seed(4)).to(dev)
        rg = types.SimpleNamespace(samples={"val": [{"transform": pose.numpy()}]}, cam_params=cam, colours={"val": table})
        res = metrics.evaluate(None, rg, ssim=False, render=lambda p: render_hierarchical_view(
            *nets, p, cam, Nc, Nf, u_c=vu_c, u_f=vu_f, controls=Controls(background=bg), **kw))
        assert res["idxs"] == [0] and abs(res["mse"][0] - float(((px[:, :3] - table) ** 2).mean())) <= 1e-6
