"""The two hand-derived ray routines per element on the GPU: the compositor's backward (nerf_amd_volume_render_backward and
the entry points that share its kernel) and the fine-pass sampler (nerf_amd_sample_pdf), each held to 2 c_ref + 4 units of
the float64 model in tests/ray_routines_model.py -- c_ref being what the oracle's own fp32 evaluation needs on the same
cases (tests/test_ray_routines_model_cpu.py).  No bound here comes from what a kernel showed."""
import numpy as np
import pytest
import torch

import ray_routines_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from nerf_simple_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


_models = {}


def _case_model(case):
    """(raw, ts, d, float64 forward) of a compositor case: formed once, shared by every test, never written to."""
    if case.id not in _models:
        raw, ts, d = M.comp_inputs(case)
        _models[case.id] = (raw, ts, d, M.forward64(raw, ts, d))
    return _models[case.id]


def _backward(dev, raw, ts, d, coef, entry="dirs"):
    """d_raw of nerf_amd_volume_render_backward through the C ABI (absent gradients as NULL); entry='rays': ``d`` is the
    [B,6] ray table of nerf_amd_volume_render_rays_backward."""
    from nerf_simple_amd import _lib
    lib, ptr = _lib.lib(), _lib.ptr
    B, N = ts.shape
    raw, ts, d = raw.to(dev).contiguous(), ts.to(dev).contiguous(), d.to(dev).contiguous()
    g = [None if c is None else c.to(dev).contiguous() for c in coef]
    d_raw = torch.full((B, N, 4), float("nan"), device=dev)
    if entry == "rays":
        _lib.check(lib.nerf_amd_volume_render_rays_backward(ptr(raw), ptr(ts), ptr(d), *[ptr(x) for x in g], ptr(d_raw), B, N,
                                                            _lib.stream_ptr(dev)), "nerf_amd_volume_render_rays_backward")
    else:
        _lib.check(lib.nerf_amd_volume_render_backward(ptr(raw), ptr(ts), ptr(d), 3, *[ptr(x) for x in g], ptr(d_raw), B, N,
                                                       _lib.stream_ptr(dev)), "nerf_amd_volume_render_backward")
    torch.cuda.synchronize(dev)
    return d_raw.cpu()


def _report(tag, worst):
    print(f"{tag}: " + ", ".join(f"{k} {v[0]:.2f} of {v[1]:.1f} ({v[2]})" for k, v in worst.items()))


def _track(worst, key, ratio, limit, cid):
    if key not in worst or ratio / limit > worst[key][0] / worst[key][1]:
        worst[key] = (ratio, limit, cid)


def test_backward_g_alpha_alone(dev):
    """d_raw[..., 3] = g e delta softplus'(sigma) per element, relative; the colour columns exactly zero.  The dense and
    threshold sets are where  (1 - a)  in place of  e = exp(-softplus(sigma) delta)  would show (a relative 2^-24 / e),
    and the last sample at sigma = -100 where softplus' underflows unless it is formed as exp(sigma) / (1 + exp(sigma))."""
    worst, failed = {}, []
    for case in M.comp_cases():
        raw, ts, d, fw = _case_model(case)
        g = M.coefs(case, "alpha")
        got = _backward(dev, raw, ts, d, g).numpy()
        want, unit = M.model_alpha(fw, g[2])
        assert (got[..., :3] == 0).all(), case.id
        checks = (("plain-" + case.set, unit, M.bound(M.C_REF_ALPHA[case.set])),
                  ("conditioned", M.EPS * M.model_backward(fw, raw, ts, g)[1][..., 3], M.bound(M.C_REF_ALPHA_COND)))
        for key, u_, limit in checks:
            r = M.element_ratio(got, want, u_)
            _track(worst, key, r, limit, case.id)
            if not r <= limit:
                failed.append((case.id, key, r, limit))
    _report("g_alpha alone, units per element", worst)
    assert not failed, failed


def test_backward_g_w_one_hot(dev):
    """g_w one-hot at sample j of each ray: -w_j ds_i / f_i in front of j, T_j ds_j at j, exactly zero behind it and in
    the colour columns; the conditioned unit of the model on the judged rays, the first-order unit on every ray."""
    worst, failed = {}, []
    for case in M.comp_cases():
        raw, ts, d, fw = _case_model(case)
        g = M.coefs(case, "w", fw)
        got = _backward(dev, raw, ts, d, g).numpy()
        want, unit = M.model_w(fw, M.pick_w_samples(fw)[0])
        assert (got[..., :3] == 0).all(), case.id
        assert (got[..., 3][unit == 0] == 0).all(), case.id
        checks = (("judged-" + case.set, unit, M.bound(M.C_REF_W[case.set])),
                  ("conditioned", M.EPS * M.model_backward(fw, raw, ts, g)[1][..., 3], M.bound(M.C_REF_W_COND)))
        for key, u_, limit in checks:
            r = M.element_ratio(got, want, u_)
            _track(worst, key, r, limit, case.id)
            if not r <= limit:
                failed.append((case.id, key, r, limit))
    _report("g_w one-hot, units per element", worst)
    assert not failed, failed


@pytest.mark.parametrize("kind", ["rgb", "disp", "acc", "all"])
def test_backward_per_ray(dev, kind):
    """g_rgb, g_disp, g_acc alone and all five together: per ray, the colour block and the sigma column separately, in
    units of EPS max_i A_i (the first-order bound, every ray) and of EPS max_i |want_i| (the ray's own largest gradient,
    the judged rays).  Entries where the oracle's fp32 autograd is not finite (an empty ray's disparity) are not judged:
    test_backward_disparity_clamp_and_empty_rays pins them."""
    worst, failed = {}, []
    for case in M.comp_cases():
        raw, ts, d, fw = _case_model(case)
        g = M.coefs(case, kind)
        got = _backward(dev, raw, ts, d, g).numpy()
        want, A = M.model_backward(fw, raw, ts, g)
        keep = np.isfinite(M.oracle_grad(raw, ts, d, g, torch.float32))
        assert np.isfinite(got[keep]).all(), case.id
        cond, plain = M.ray_ratios(got, want, A, keep)
        for key, r, limit in (("conditioned", float(cond.max()), M.bound(M.C_REF_RAY[kind])),
                              ("plain", float(np.nanmax(plain, initial=0.0)), M.bound(M.C_REF_RAY_PLAIN[kind]))):
            _track(worst, key, r, limit, case.id)
            if not r <= limit:
                failed.append((case.id, key, r, limit))
    _report(f"g_{kind}, units per ray", worst)
    assert not failed, failed


def test_backward_disparity_clamp_and_empty_rays(dev):
    """g_disp alone where the disparity has no slope.  Clamp branch (depth / acc <= 1e-10): autograd gives zero (the
    constant wins torch.max) and so does the kernel.  Empty ray (acc == 0, disparity = 1 / max(1e-10, 0/0) = NaN):
    autograd gives NaN in the sigma column (NaN x softplus' = NaN even where softplus' is 0) and 0 in the colours; the
    kernel gives ZERO throughout -- its documented convention (include/nerf_amd.h): the forward's NaN disparity already
    says that the ray is empty, and a NaN written into d_raw would reach every weight of the network."""
    raw, ts, d, g_disp, kinds = M.disp_edge_inputs()
    g = [None, g_disp, None, None, None]
    got = _backward(dev, raw, ts, d, g).numpy()
    want, A = M.model_backward(M.forward64(raw, ts, d), raw, ts, g)
    plain = np.array([k == "plain" for k in kinds])
    assert (got[~plain] == 0).all(), [k for k, row in zip(kinds, got) if not (row == 0).all()]
    cond, _ = M.ray_ratios(got[plain], want[plain], A[plain])
    assert cond.max() <= M.bound(M.C_REF_RAY["disp"]), cond.max()
    assert (np.abs(got[plain][..., 3]).max(axis=1) > 0).all()


@pytest.mark.parametrize("k", range(len(M.NONFINITE_SHAPES)))
def test_backward_non_finite_inputs(dev, k):
    """The training case (rgb-only upstream) on NaN, +-inf sigma and NaN, inf, 1e30 colours: NaNs exactly where the
    oracle's fp32 autograd has them, the finite entries to the per-ray rule, and the rays without a non-finite value bit
    for bit what they are when run alone -- a diverged ray stays loud and stays in its ray."""
    raw, ts, d, g_rgb, clean = M.nonfinite_inputs(k)
    g = [g_rgb, None, None, None, None]
    got = _backward(dev, raw, ts, d, g)
    alone = _backward(dev, raw[clean], ts[clean], d[clean], [g_rgb[clean], None, None, None, None])
    assert torch.equal(got[clean], alone) and bool(torch.isfinite(alone).all())
    got = got.numpy()
    ref32, ref64 = M.oracle_grad(raw, ts, d, g, torch.float32), M.oracle_grad(raw, ts, d, g, torch.float64)
    differ = np.isnan(got) != np.isnan(ref32)
    assert not differ.any(), (int(differ.sum()), np.argwhere(differ)[:5].tolist(), got[differ][:5], ref32[differ][:5])
    with np.errstate(all="ignore"):
        A = M.model_backward(M.forward64(raw, ts, d), raw, ts, g)[1]
    keep = M.nonfinite_keep(ref32, ref64)
    assert np.isfinite(got[keep]).all()
    cond, _ = M.ray_ratios(got, ref64, A, keep)
    print(f"non-finite inputs {M.NONFINITE_SHAPES[k]}: {cond.max():.2f} of {M.bound(M.C_REF_NONFINITE):.1f} units")
    assert cond.max() <= M.bound(M.C_REF_NONFINITE), cond.max()


SEAM_CASES = [c for c in M.comp_cases() if c.set == "dense" and c.s == 15.0 and c.N in (2, 63, 65, 129, 512)] + \
             [c for c in M.comp_cases() if c.set == "threshold" and c.N in (64, 128)]


@pytest.mark.parametrize("case", SEAM_CASES, ids=lambda c: c.id)
def test_entry_points_share_the_kernel(dev, case):
    """At the chunk seams: autograd through utils.rendering.volume_render, nerf_amd_volume_render_rays_backward and
    nerf_amd_volume_render_mse_backward (g_rgb = 2 (rgb - target) / (3 B)) give the bits of
    nerf_amd_volume_render_backward."""
    from nerf_simple_amd import _lib
    from nerf_simple_amd.utils.rendering import volume_render
    lib, ptr = _lib.lib(), _lib.ptr
    raw, ts, d, _ = _case_model(case)
    B, N = ts.shape
    g = M.coefs(case, "all")
    gen = torch.Generator().manual_seed(case.seed + 1)
    rays = torch.cat([torch.randn(B, 3, generator=gen), d], dim=1)
    dn = d / torch.norm(d, dim=1, keepdim=True)               # the kernels' own normalisation, bit for bit
    base = _backward(dev, raw, ts, dn, g)
    assert torch.equal(_backward(dev, raw, ts, rays, g, entry="rays"), base)
    r = raw.to(dev).requires_grad_(True)
    M.loss_of(volume_render(r, ts.to(dev), dn.to(dev)), g).backward()
    assert torch.equal(r.grad.cpu(), base)
    # the fused MSE form against the rgb-only backward fed with the loss gradient of its own forward
    target = torch.rand(B, 3, generator=gen).to(dev)
    raw_d, ts_d, rays_d = raw.to(dev).contiguous(), ts.to(dev).contiguous(), rays.to(dev).contiguous()
    rgb, d_mse = torch.empty(B, 3, device=dev), torch.full((B, N, 4), float("nan"), device=dev)
    _lib.check(lib.nerf_amd_volume_render_mse_backward(ptr(raw_d), ptr(ts_d), ptr(rays_d), ptr(target), ptr(rgb), ptr(d_mse), B, N,
                                                       _lib.stream_ptr(dev)), "nerf_amd_volume_render_mse_backward")
    with torch.no_grad():
        assert torch.equal(volume_render(raw_d, ts_d, dn.to(dev))[0], rgb)
    scale = torch.tensor(1.0) / (torch.tensor(3.0) * torch.tensor(float(B)))
    g_rgb = 2.0 * (rgb - target) * scale.to(dev)
    assert torch.equal(_backward(dev, raw, ts, rays, [g_rgb, None, None, None, None], entry="rays"), d_mse.cpu())


@pytest.mark.parametrize("Nc,Nf", [(66, 65), (130, 129), (256, 256)])
def test_coarse_head_at_the_seams(dev, Nc, Nf):
    """nerf_amd_volume_render_mse_backward_pdf = nerf_amd_volume_render_mse_backward + nerf_amd_sample_pdf on the forward's
    weights, bit for bit, on dense raw values at the shapes where the register sort and the cdf scan change path."""
    from nerf_simple_amd import _lib
    lib, ptr = _lib.lib(), _lib.ptr
    st = _lib.stream_ptr(dev)
    B = 37
    gen = torch.Generator().manual_seed(100 * Nc + Nf)
    raw = torch.randn(B, Nc, 4, generator=gen)
    raw[..., 3] = 15.0 * raw[..., 3] + 7.5
    ts = M.O.sample_ts(torch.rand(B, Nc, generator=gen))
    rays, target, u = torch.randn(B, 6, generator=gen), torch.rand(B, 3, generator=gen), torch.rand(B, Nf, generator=gen)
    raw, ts, rays, target, u = [x.contiguous().to(dev) for x in (raw, ts, rays, target, u)]
    f32 = dict(dtype=torch.float32, device=dev)
    rgb_ref, d_ref = torch.empty(B, 3, **f32), torch.empty(B, Nc, 4, **f32)
    _lib.check(lib.nerf_amd_volume_render_mse_backward(ptr(raw), ptr(ts), ptr(rays), ptr(target), ptr(rgb_ref), ptr(d_ref), B, Nc, st),
               "nerf_amd_volume_render_mse_backward")
    outs = [torch.empty(s_, **f32) for s_ in ((B, 3), (B,), (B, Nc), (B,), (B, Nc))]
    _lib.check(lib.nerf_amd_volume_render_rays(ptr(raw), ptr(ts), ptr(rays), *[ptr(x) for x in outs], B, Nc, st),
               "nerf_amd_volume_render_rays")
    ts_ref = torch.empty(B, Nc + Nf, **f32)
    _lib.check(lib.nerf_amd_sample_pdf(ptr(ts), ptr(outs[4]), ptr(u), 0, 0, 0, ptr(ts_ref), B, Nc, Nf, st), "nerf_amd_sample_pdf")
    rgb, d_raw, ts_out = [torch.full(s_, float("nan"), **f32) for s_ in ((B, 3), (B, Nc, 4), (B, Nc + Nf))]
    _lib.check(lib.nerf_amd_volume_render_mse_backward_pdf(ptr(raw), ptr(ts), ptr(rays), ptr(target), ptr(u), 0, 0, 0, ptr(rgb),
                                                           ptr(d_raw), ptr(ts_out), B, Nc, Nf, st),
               "nerf_amd_volume_render_mse_backward_pdf")
    torch.cuda.synchronize(dev)
    assert torch.equal(rgb, rgb_ref) and torch.equal(d_raw, d_ref) and torch.equal(ts_out, ts_ref)


@pytest.mark.parametrize("N", [3, 64, 65, 256])
def test_four_backward_kernels_write_the_same_bytes(dev, N):
    """The compositor's backward walk is one routine (csrc/composite_backward_device.h): from the same raw and gt, under an
    all-live mask, the dense MSE backward, the masked backward fed the g_rgb nerf_amd_mse_loss forms, the capped head at
    C = B N and the capped pdf head at C = B N (Nf = 8) write the same d_raw bytes.  N: one partial chunk, one full chunk, a
    chunk seam, and the pdf head's four-chunk limit.  Then, under a sparse mask, the three masked launches among themselves:
    the same d_raw and rgb bytes at C = P', and the two capped heads the same bytes at C = P' - 3."""
    from nerf_simple_amd import _lib
    lib, ptr = _lib.lib(), _lib.ptr
    st = _lib.stream_ptr(dev)
    B, Nf, TS_GIVEN = 5, 8, _lib.FLAG_TS_GIVEN
    gen = torch.Generator().manual_seed(7000 + N)
    raw = torch.randn(B, N, 4, generator=gen)
    raw[..., 3] = 15.0 * raw[..., 3] + 7.5
    ts = M.O.sample_ts(torch.rand(B, N, generator=gen))
    rays, gt, u_f = torch.randn(B, 6, generator=gen), torch.rand(B, 3, generator=gen), torch.rand(B, Nf, generator=gen)
    raw, ts, rays, gt, u_f = [x.contiguous().to(dev) for x in (raw, ts, rays, gt, u_f)]
    i = torch.arange(((N + 63) // 64) * 64).view(-1, 64)
    words = ((i < N).long() << (i % 64)).sum(1)                      # bit b of word q: sample 64 q + b exists
    mask = words.expand(B, -1).contiguous().to(dev)
    offsets = (torch.arange(B + 1, dtype=torch.int64) * N).to(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    nan = lambda *shape: torch.full(shape, float("nan"), **f32)      # noqa: E731
    rgb, d_dense = nan(B, 3), nan(B, N, 4)
    _lib.check(lib.nerf_amd_volume_render_mse_backward(ptr(raw), ptr(ts), ptr(rays), ptr(gt), ptr(rgb), ptr(d_dense), B, N, st),
               "nerf_amd_volume_render_mse_backward")
    jit = (ptr(rays), ptr(ts), None, TS_GIVEN, 0, 0, ptr(mask), ptr(offsets))
    loss, g_rgb, d_masked = nan(), nan(B, 3), nan(B * N, 4)
    _lib.check(lib.nerf_amd_mse_loss(ptr(rgb), ptr(gt), ptr(loss), ptr(g_rgb), B * 3, st), "nerf_amd_mse_loss")
    _lib.check(lib.nerf_amd_volume_render_masked_backward(ptr(raw), *jit, ptr(g_rgb), None, None, None, None, ptr(d_masked), B, N, st),
               "nerf_amd_volume_render_masked_backward")
    rgb_head, d_head = nan(B, 3), nan(B * N, 4)
    _lib.check(lib.nerf_amd_volume_render_masked_mse_backward(ptr(raw), *jit, ptr(gt), ptr(rgb_head), ptr(d_head), B * N, B, N, st),
               "nerf_amd_volume_render_masked_mse_backward")
    rgb_pdf, d_pdf, ts_out = nan(B, 3), nan(B * N, 4), nan(B, N + Nf)
    _lib.check(lib.nerf_amd_volume_render_masked_mse_backward_pdf(ptr(raw), *jit, ptr(gt), ptr(u_f), ptr(rgb_pdf), ptr(d_pdf),
                                                                  ptr(ts_out), B * N, B, N, Nf, st),
               "nerf_amd_volume_render_masked_mse_backward_pdf")
    torch.cuda.synchronize(dev)
    want = d_dense.view(torch.int32).view(B * N, 4)
    assert torch.isfinite(d_dense).all() and (d_dense != 0).any()
    assert torch.equal(rgb_head, rgb) and torch.equal(rgb_pdf, rgb)
    for name, d in (("masked backward", d_masked), ("capped head", d_head), ("capped pdf head", d_pdf)):
        assert torch.equal(d.view(torch.int32), want), name

    # A second, sparse mask, compared among the three masked launches (one kernel, csrc/occupancy_train.hip, under its three
    # heads): ray 0 dead -- the nothing-kept early out in both LDS layouts --, ray 1 live at its last sample only, rays 2 .. 4
    # live at i with (7 i + 3 ray) % 5 < 2, across the mask word boundary from N = 65 on.
    s = np.arange(N)
    live = np.zeros((B, N), bool)
    live[1, N - 1] = True
    for r in range(2, B):
        live[r] = (7 * s + 3 * r) % 5 < 2
    counts = live.sum(1)
    P = int(counts.sum())
    assert P >= 4 and (N != 3 or counts.tolist() == [0, 1, 2, 1, 1])
    assert N < 65 or any(live[r, :64].any() and live[r, 64:].any() for r in range(B))
    words2 = np.zeros((B, (N + 63) // 64), np.uint64)
    for r, k in zip(*np.nonzero(live)):
        words2[r, k // 64] |= np.uint64(1) << np.uint64(k % 64)
    mask2 = torch.from_numpy(words2.view(np.int64)).to(dev)
    offsets2 = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev)
    raw_live = raw.view(B * N, 4)[torch.from_numpy(live.reshape(-1)).to(dev)].contiguous()
    jit2 = (ptr(rays), ptr(ts), None, TS_GIVEN, 0, 0, ptr(mask2), ptr(offsets2))
    rgb_fwd, disp, acc = nan(B, 3), nan(B), nan(B)
    _lib.check(lib.nerf_amd_volume_render_masked(ptr(raw_live), *jit2, ptr(rgb_fwd), ptr(disp), None, ptr(acc), None, B, N, st),
               "nerf_amd_volume_render_masked")
    g_rgb2, d_eager = nan(B, 3), nan(P, 4)
    _lib.check(lib.nerf_amd_mse_loss(ptr(rgb_fwd), ptr(gt), ptr(loss), ptr(g_rgb2), B * 3, st), "nerf_amd_mse_loss")
    _lib.check(lib.nerf_amd_volume_render_masked_backward(ptr(raw_live), *jit2, ptr(g_rgb2), None, None, None, None, ptr(d_eager), B, N,
                                                          st), "nerf_amd_volume_render_masked_backward")

    def heads(C):
        """(rgb, d_raw[C]) of the capped head and of the capped pdf head at capacity C"""
        rgb_a, d_a, rgb_b, d_b, ts_b = nan(B, 3), nan(C, 4), nan(B, 3), nan(C, 4), nan(B, N + Nf)
        _lib.check(lib.nerf_amd_volume_render_masked_mse_backward(ptr(raw_live), *jit2, ptr(gt), ptr(rgb_a), ptr(d_a), C, B, N, st),
                   "nerf_amd_volume_render_masked_mse_backward")
        _lib.check(lib.nerf_amd_volume_render_masked_mse_backward_pdf(ptr(raw_live), *jit2, ptr(gt), ptr(u_f), ptr(rgb_b), ptr(d_b),
                                                                      ptr(ts_b), C, B, N, Nf, st),
                   "nerf_amd_volume_render_masked_mse_backward_pdf")
        torch.cuda.synchronize(dev)
        assert torch.isfinite(ts_b).all()
        return rgb_a.view(torch.int32), d_a.view(torch.int32), rgb_b.view(torch.int32), d_b.view(torch.int32)

    rgb_a, d_a, rgb_b, d_b = heads(P)                                # C = P': nothing is cut
    assert torch.isfinite(d_eager).all() and (d_eager != 0).any() and (rgb_fwd[0] == 0).all()
    assert torch.equal(rgb_a, rgb_fwd.view(torch.int32)) and torch.equal(rgb_b, rgb_a)
    assert torch.equal(d_a, d_eager.view(torch.int32)) and torch.equal(d_b, d_a)
    rgb_a, d_a, rgb_b, d_b = heads(P - 3)                            # the clamp cuts inside a ray
    first = np.cumsum(counts) - counts
    assert ((first < P - 3) & (P - 3 < first + counts)).any()
    assert torch.equal(rgb_b, rgb_a) and torch.equal(d_b, d_a)
    assert torch.isfinite(d_a.view(torch.float32)).all() and torch.isfinite(rgb_a.view(torch.float32)).all()


@pytest.mark.parametrize("case", M.pdf_cases(), ids=lambda c: c.id)
def test_sample_pdf_per_ray(dev, case):
    """nerf_amd_sample_pdf with explicit u: ascending, the Nc coarse positions present bit for bit, and every ray without
    a kink within 2 c_ref + 4 of its largest unit of the float64 model, sorted rows in sup norm."""
    from nerf_simple_amd.utils.rendering import sample_pdf
    ts, w, u = M.pdf_inputs(case)
    want, unit, kink = M.model_pdf(ts, w, u)
    got = sample_pdf(ts.to(dev), w.to(dev), case.Nf, u=u.to(dev)).cpu()
    assert got.shape == (M.PDF_B, case.Nc + case.Nf)
    assert bool((got[:, 1:] >= got[:, :-1]).all()), "positions must be ascending"
    # ascending rows: the coarse positions are present when each is found at its insertion point
    at = torch.searchsorted(got, ts.contiguous()).clamp(max=got.shape[1] - 1)
    assert torch.equal(torch.gather(got, 1, at), ts), "a coarse position is missing"
    r = M.pdf_ratios(got.numpy(), want, unit)
    assert kink.sum() <= M.kink_cap(case) * M.PDF_B
    print(f"{case.id}: {r[~kink].max():.2f} of {M.bound(M.C_REF_PDF):.1f} units, {int(kink.sum())} kink rays left out")
    assert r[~kink].max() <= M.bound(M.C_REF_PDF), (int(r[~kink].argmax()), r[~kink].max())
