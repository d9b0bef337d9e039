"""tests/adam_model.py checked on the CPU: the scalar rule against exact arithmetic and the figures of the issue, the element
model against torch.optim.Adam in float64, the bounds against fp32 emulations of the kernel's fused and unfused spellings,
and the bounds' bite -- a bias correction formed from the unrounded beta leaves them."""
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import torch

import adam_model as A

BETAS, EPS, LR = (0.9, 0.999), 1e-8, 5e-4
STEPS = (1, 2, 16, 17, 100, 1000)


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def old_graphed_scalars(t):
    """What GraphedTrainStep._set_hyper formed before there was one rule: corrections from the Python doubles."""
    b1, b2 = BETAS
    return np.float32(1.0 - b1 ** t), np.float32((1.0 - b2 ** t) ** 0.5)


def test_scalars_are_the_headers_rule_exactly():
    """At every quoted step: the fp32 betas, and corrections equal to the EXACT 1 - b^t (rational arithmetic) and its square
    root (60 decimal digits) rounded once to fp32 -- the double intermediate of the header's rule changes no bit here."""
    getcontext().prec = 60
    for t in STEPS:
        s = A.scalars(LR, BETAS, EPS, t)
        assert s.dtype == np.float32 and s.shape == (6,)
        assert s[0] == np.float32(LR) and s[1] == np.float32(0.9) and s[2] == np.float32(0.999) and s[3] == np.float32(EPS)
        b1, b2 = Fraction(float(s[1])), Fraction(float(s[2]))
        assert s[4] == np.float32(float(1 - b1 ** t)), t
        x = 1 - b2 ** t
        root = (Decimal(x.numerator) / Decimal(x.denominator)).sqrt()
        assert s[5] == np.float32(float(root)), t
        # the C ABI's spelling: pow and sqrt of doubles
        assert s[4] == np.float32(1.0 - math.pow(float(s[1]), t)) and s[5] == np.float32(math.sqrt(1.0 - math.pow(float(s[2]), t)))


def test_scalars_reproduce_the_quoted_figures():
    """t = 1: 0.031622574 by the rule, 0.031622775 from the unrounded beta, 54 ulps = 6.4e-6 apart; 50 ... 77 ulps at every
    quoted step up to 1000; the first correction 1 ... 3 ulps apart over the first steps."""
    s1 = A.scalars(LR, BETAS, EPS, 1)
    old4, old5 = old_graphed_scalars(1)
    assert f"{float(s1[5]):.9f}" == "0.031622574" and f"{float(old5):.9f}" == "0.031622775"
    assert ulps(s1[5], old5) == 54
    assert abs(float(old5) / float(s1[5]) - 1 - 6.4e-6) < 0.05e-6
    for t in STEPS:
        s = A.scalars(LR, BETAS, EPS, t)
        o4, o5 = old_graphed_scalars(t)
        print(f"t={t} bc1 {s[4]!r} (doubles: {o4!r}, {ulps(s[4], o4)} ulps)  bc2s {s[5]!r} (doubles: {o5!r}, {ulps(s[5], o5)} ulps)")
        assert 50 <= ulps(s[5], o5) <= 77, t
        if t <= 17:
            assert 1 <= ulps(s[4], o4) <= 3, t


def test_hyper_words():
    w = A.hyper_words(A.scalars(LR, BETAS, EPS, 17), 17)
    assert w.dtype == np.int32 and list(w[6:]) == [17, 0] and w[:6].view(np.float32)[4] == A.scalars(LR, BETAS, EPS, 17)[4]
    assert list(A.hyper_words(np.zeros(6, np.float32), (1 << 32) + 5)[6:]) == [5, 1]


def inputs(n, seed, zero_moments=False):
    """Gradients randn 10^U(-8, 0) (the suite's Adam gradients), parameters randn 10^U(-6, 0) (small ones beside large ones:
    the update shows in a small parameter's low bits), moments as a few steps on such gradients leave them."""
    gen = np.random.default_rng(seed)
    g = (gen.standard_normal(n) * 10.0 ** gen.uniform(-8, 0, n)).astype(np.float32)
    p = (gen.standard_normal(n) * 10.0 ** gen.uniform(-6, 0, n)).astype(np.float32)
    if zero_moments:
        return p, np.zeros(n, np.float32), np.zeros(n, np.float32), g
    g0 = (gen.standard_normal(n) * 10.0 ** gen.uniform(-8, 0, n)).astype(np.float32)
    return p, (0.1 * g0).astype(np.float32), (0.001 * g0 * g0).astype(np.float32), g


def plant(p, m, v, g, at):
    """The corners of the GPU test at the indices ``at``: a zero gradient on a zero second moment, |g| = 1e-23 (its square
    underflows), g = 1e19 (the issue's; its square and (1 - b2) g^2 stay finite in fp32) and g = 1e21 ((1 - b2) g^2 overflows)."""
    vals = (0.0, 1e-23, -1e-23, 1e19, 1e21, -1e21)
    for i, k in enumerate(at):
        g[k] = vals[i % len(vals)]
        if vals[i % len(vals)] == 0.0 or abs(vals[i % len(vals)]) == 1e-23:
            v[k] = 0.0
            m[k] = 0.0


def test_model_tracks_torch_adam_in_float64():
    """20 steps with the learning rate decayed every step, carried in float64 with the scalars unrounded: the model's
    expression is torch.optim.Adam's.  20 steps of fewer than 16 float64 operations each: 320 x 2^-53 of the largest value."""
    n, b1, b2, eps = 4096, A.f32(0.9), A.f32(0.999), A.f32(1e-8)
    p0, _, _, _ = inputs(n, 1)
    ref = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([ref], lr=LR, betas=(b1, b2), eps=eps)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    lr, decay = LR, (1e-4 / 5e-4) ** (1 / 20)
    for t in range(1, 21):
        g = inputs(n, 100 + t)[3].astype(np.float64)
        ref.grad = torch.tensor(g)
        for pg in opt.param_groups:
            pg["lr"] = lr
        opt.step()
        bc1, bc2s = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
        p, m, v = A.element64(p, m, v, g, b1, b2, eps, bc2s, 1.0 - b1, 1.0 - b2, lr / bc1)[:3]
        lr *= decay
    state = opt.state[ref]
    tol = 320 * 2.0 ** -53
    for name, got, want in (("p", p, ref.detach().numpy()), ("m", m, state["exp_avg"].numpy()), ("v", v, state["exp_avg_sq"].numpy())):
        err = float(np.max(np.abs(got - want)))
        print(f"{name}: max |model - torch64| = {err:.3g} (allowed {tol * float(np.max(np.abs(want))):.3g})")
        assert err <= tol * float(np.max(np.abs(want))), name


def test_bounds_hold_for_both_spellings():
    """numpy fp32 emulations of adam_element with every a * b + c unfused and fused, three chained steps at t = 1, 2, 1000 and
    one with lr = 0, the corners planted: every element inside its bound, the overflowed ones exactly inf / unchanged."""
    n = 70001
    for fused in (False, True):
        p, m, v, g = inputs(n, 7, zero_moments=True)
        at = list(range(0, 12)) + list(range(n - 6, n))
        for t, lr in ((1, LR), (2, LR), (1000, LR), (1000, 0.0)):
            g = inputs(n, 7 + t)[3]
            plant(p, m, v, g, at)
            s = A.scalars(lr, BETAS, EPS, t)
            res = A.step(p, m, v, g, s)
            assert not res.ambiguous.any()
            assert list(np.flatnonzero(res.v_inf)) == [k for i, k in enumerate(at) if i % 6 >= 4]
            pn, mn, vn = A.emulate(p, m, v, g, s, fused)
            r = A.ratios(res, pn, mn, vn)
            print(f"fused={fused} t={t} lr={lr}: worst ratios {r}")
            assert max(r.values()) <= 1.0, (fused, t, r)
            assert np.all(np.isposinf(vn[res.v_inf])) and np.array_equal(pn[res.v_inf], p[res.v_inf])
            if lr == 0.0:
                assert np.array_equal(pn, p)
            p, m, v = pn, mn, vn


def test_bounds_are_not_trivial():
    """The same step with bc2s = sqrt(1 - 0.999**t) -- the correction from the unrounded beta, 54 ulps away -- leaves the p
    bound at t = 1; so does a bias correction of the neighbouring step, and an update applied twice leaves all three."""
    n = 70001
    p, m, v, g = inputs(n, 7, zero_moments=True)
    s = A.scalars(LR, BETAS, EPS, 1)
    res = A.step(p, m, v, g, s)
    wrong = s.copy()
    wrong[5] = np.float32(math.sqrt(1.0 - 0.999 ** 1))
    assert ulps(wrong[5], s[5]) == 54
    r = A.ratios(res, *A.emulate(p, m, v, g, wrong, False))
    print(f"bc2s from the unrounded beta: {r}")
    assert r["p"] > 1.0 and r["m"] <= 1.0 and r["v"] <= 1.0
    r = A.ratios(res, *A.emulate(p, m, v, g, A.scalars(LR, BETAS, EPS, 2), False))
    assert r["p"] > 1.0
    once = A.emulate(p, m, v, g, s, False)
    r = A.ratios(res, *A.emulate(*once, g, s, False))
    assert min(r.values()) > 1.0
