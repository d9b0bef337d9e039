"""Per-element models of the two hand-derived ray routines (test infrastructure; uses the oracle): the compositor's
backward (csrc/composite.hip, composite_backward_kernel) and the fine-pass sampler (csrc/sample_pdf_device.h,
nerf_pdf::sample_ray).

The rule is tests/error_model.py's fp32 rule, per element instead of per tensor: the value is the float64 evaluation of
the oracle (oracle.volume_render under autograd, oracle.sample_pdf) on the fp32 inputs; the oracle's own fp32 evaluation
sits c_ref UNITS from it (the largest ratio over every committed case, measured on the CPU and recorded below); the
kernel, another fp32 evaluation of the same expression in another order, may sit  bound(c_ref) = 2 c_ref + 4  units
from it.  A unit is a stated function of the float64 intermediates -- never of a kernel's output.  EPS = 2^-24.

Compositor backward, d loss / d raw[B,N,4] for loss = sum_k <coef_k, output_k>:

  'alpha' (g_alpha alone): d_raw[..., 3] = g e delta softplus'(sigma), e = exp(-softplus(sigma) delta); colours exactly 0.
          unit_i = EPS |want_i|  (+ the subnormal terms below).
  'w'     (g_w alone, one-hot at sample j of each ray): elements i > j and the colours exactly 0; i < j: -w_j ds_i / f_i;
          i = j: T_j ds_j  (ds = e delta softplus', f = 1 - alpha + 1e-10).  unit_i = u_i |want_i| with the conditioned
          u_i = EPS (1 + 1/|alpha_j| + sum_{k<=j} (1 + 1/f_k) + 1/f_i): every f_k is formed with an absolute rounding of
          EPS, T_j is their product, alpha_j = 1 - e_j likewise.  A ray is JUDGED when max_{i<=j} u_i <= 2^-10: beyond
          that the fp32 value of a saturated factor (f = 1e-10 against e + 1e-10) says nothing about the float64 one.
          j is picked from the float64 forward alone: the largest index at or below the ray's target
          (0, 1, 62, 63, 64, 65, N-2, N-1 in turn) that is judged and has alpha_j >= 1e-3, if there is one.
  'rgb', 'disp', 'acc', 'all' (per ray, colour block and sigma column separately): unit = EPS max_i |want_i| of the ray.

  Subnormal terms (the format's, not the algorithm's): below 2^-126 an fp32 value carries an absolute rounding of
  2^-150, so every per-element unit gets + 2^-149, and softplus'(sigma) = exp(sigma) / (1 + exp(sigma)) below 2^-126
  (sigma < -87.3) carries the relative error 2^-150 / softplus' into its element: unit_i += |want_i| 2^-150 / softplus'_i.

Sampler, per new sample: z = b0 + (u - c0) / denom (b1 - b0); unit = EPS [(b1 - b0) (1 + (c1 + u) / denom) + |z|] (the
cdf's rounding, of the order EPS c1, divided by the bin's mass, plus the rounding of z itself); KINK where denom = c1 - c0
is within  (8 + Nc/64) EPS c1 + EPS 1e-5  of the 1e-5 switch to denom = 1, which an fp32 prefix sum can cross (kink_window),
and where u is within that of the upper edge of a bin under the switch (z jumps from b0 to b1 there).  Rows
[B, Nc+Nf] are compared SORTED, in sup norm per ray, in units of the ray's largest unit: sorting is 1-Lipschitz in that
norm, so no matching of elements is needed.  Rays with a kink are left out (kink_cap: at most 2 % of a case's rays, more
only where opaque rays with exact floor bins sit at the switch by construction).

The constants C_REF_* were written by

    python tests/ray_routines_model.py            (about half a minute on a CPU; prints the dictionaries below)

and tests/test_ray_routines_model_cpu.py asserts that the oracle's fp32 evaluation stays inside them on every case.
"""
import os
import sys
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import nerf_oracle as O  # noqa: E402

EPS = 2.0 ** -24
SUBNORMAL = 2.0 ** -149             # spacing of fp32 below FLT_MIN = 2^-126
FLT_MIN = 2.0 ** -126
JUDGED_MAX_UNIT = 2.0 ** -10        # 'w' rows with a larger conditioned unit are not judged
PLAIN_JUDGED = 16.0                 # 'rgb' ... 'all': the plain per-ray scale is judged where the first-order bound is within 16x of it
KINK_CAP = 0.02                     # at most this share of a sampler case's rays may carry a kink
NAMES = ("rgb", "disp", "alpha", "acc", "w")


def bound(c_ref):
    """tests/error_model.py's fp32 rule: FACTOR_32 x the reference's own error + 4 units for the final roundings."""
    return 2.0 * c_ref + 4.0


# ---- measured on the CPU by `python tests/ray_routines_model.py`: the float32 oracle against the float64 model, the
# largest ratio over every committed case, rounded up to two digits ----
# 'alpha', unit EPS |want| (the exponential's rounded argument x is not in this unit: the sets differ by their largest x)
C_REF_ALPHA = {"benign": 24.0, "dense": 87.0, "threshold": 101.0}
C_REF_ALPHA_COND = 2.7              # 'alpha', unit EPS A (model_backward): x is in the unit
C_REF_W = {"benign": 0.43, "dense": 0.91, "threshold": 0.44}     # 'w', the conditioned unit u |want| on the judged rays
C_REF_W_COND = 1.8                  # 'w', unit EPS A, every ray
# 'rgb' ... 'all' per ray and block: unit EPS max_i A_i on every ray / EPS max_i |want_i| on the judged rays
C_REF_RAY = {"rgb": 1.8, "disp": 1.2, "acc": 1.3, "all": 1.5}
C_REF_RAY_PLAIN = {"rgb": 24.0, "disp": 5.5, "acc": 2.0, "all": 24.0}
C_REF_NONFINITE = 0.66              # rgb-only on non-finite inputs, unit EPS max_i A_i over the finite entries
C_REF_PDF = 4.2                     # sampler, the ray's largest unit, rays without a kink
# 'w' cases in which fewer than half of the rays can be judged: at N <= 3 with a coincident pair or a dense set the first
# sample is empty or saturated, and the last one (delta = 1e10) always is; single rays are all or nothing
W_UNDERJUDGED = ("dense15-N2-B1", "dense30-N2-B5", "threshold3-N2-B37", "dense8-N3-B1", "dense15-N3-B5", "dense30-N3-B37",
                 "dense30-N63-B1")


# --------------------------------------------------------------------------------------------------------------------
# compositor backward: cases and inputs
# --------------------------------------------------------------------------------------------------------------------
CompCase = namedtuple("CompCase", "id set s B N coincident seed")
COMP_N = (2, 3, 63, 64, 65, 128, 129, 300, 512)
COMP_B = (1, 5, 37)
COMP_SETS = (("benign", 1.0), ("benign", 3.0), ("dense", 8.0), ("dense", 15.0), ("dense", 30.0), ("threshold", 3.0))
THRESHOLD_SIGMAS = (19.9, 20.0, 20.1, -19.9, 100.0, -100.0, 1e4, -1e4)
W_TARGETS = (0, 1, 62, 63, 64, 65, -2, -1)


def comp_cases():
    """Every N with every density set; B and the coincident pair cycle so that each N meets each B and each set both."""
    cases = []
    for a, N in enumerate(COMP_N):
        for b, (name, s) in enumerate(COMP_SETS):
            k = len(cases)
            cases.append(CompCase(f"{name}{int(s)}-N{N}-B{COMP_B[(a + b) % 3]}", name, s, COMP_B[(a + b) % 3], N,
                                  (a + b // 3) % 2 == 1, 5000 + k))
    return cases


def comp_inputs(case):
    """raw [B,N,4], ts [B,N], dirs [B,3] in fp32: sorted uniform positions in [2, 6] (one coincident pair per ray in the
    cases that ask for it), randn directions and colours, sigma = s N(0,1) + s/2; the threshold set replaces 30 % of them
    by values at and around the softplus threshold, huge and hugely negative."""
    g = torch.Generator().manual_seed(case.seed)
    B, N = case.B, case.N
    raw = torch.randn(B, N, 4, generator=g)
    raw[..., 3] = case.s * raw[..., 3] + case.s / 2
    if case.set == "threshold":
        pick = torch.rand(B, N, generator=g) < 0.3
        vals = torch.tensor(THRESHOLD_SIGMAS)[torch.randint(0, len(THRESHOLD_SIGMAS), (B, N), generator=g)]
        raw[..., 3] = torch.where(pick, vals, raw[..., 3])
    ts = torch.sort(torch.rand(B, N, generator=g) * 4 + 2, dim=1).values
    if case.coincident:
        k = max(1, N // 2)
        ts[:, k] = ts[:, k - 1]
    d = torch.randn(B, 3, generator=g)
    return raw, ts, d


def forward64(raw, ts, d):
    """The float64 intermediates of oracle.volume_render on the fp32 inputs, each formed as the oracle forms it."""
    raw, ts, d = raw.double(), ts.double(), d.double()
    delta = ts[:, 1:] - ts[:, :-1]
    delta = torch.cat((delta, 1e10 * torch.ones_like(delta[:, :1])), dim=1) * torch.norm(d[..., None, :], dim=-1)
    sigma = raw[..., 3]
    z = torch.exp(sigma)
    spd = torch.where(sigma > 20, torch.ones_like(z), z / (z + 1))           # softplus', as torch's backward forms it
    e = torch.exp(-F.softplus(sigma) * delta)
    alpha = 1 - e
    f = 1. - alpha + 1e-10
    T = torch.cumprod(torch.cat([torch.ones_like(f[:, :1]), f], -1), -1)[:, :-1]
    return dict(delta=delta, spd=spd, e=e, alpha=alpha, f=f, T=T, w=alpha * T, ds=e * delta * spd)


def _subnormal_terms(want, spd):
    rel = torch.where((spd < FLT_MIN) & (spd > 0), (SUBNORMAL / 2) / spd.clamp_min(1e-300), torch.zeros_like(spd))
    return want.abs() * rel + SUBNORMAL


def pick_w_samples(fw):
    """j[B] for the one-hot g_w, and judged[B], from the float64 forward alone (see the module docstring)."""
    alpha, f = fw["alpha"], fw["f"]
    B, N = alpha.shape
    common = EPS * (1 + 1 / alpha.abs().clamp_min(1e-300) + torch.cumsum(1 + 1 / f, dim=1))       # [B,N] as a function of j
    worst = common + EPS * torch.cummax(1 / f, dim=1).values                                      # max_{i<=j} u_i
    ok = worst <= JUDGED_MAX_UNIT
    j, judged = torch.empty(B, dtype=torch.long), torch.zeros(B, dtype=torch.bool)
    for r in range(B):
        tgt = W_TARGETS[r % len(W_TARGETS)]
        tgt = min(tgt if tgt >= 0 else max(N + tgt, 0), N - 1)
        cand = [k for k in range(tgt, -1, -1) if ok[r, k] and alpha[r, k] >= 1e-3] or [k for k in range(tgt, -1, -1) if ok[r, k]]
        j[r] = cand[0] if cand else tgt
        judged[r] = bool(cand)
    return j, judged


def coefs(case, kind, fw=None):
    """The upstream gradients (g_rgb [B,3], g_disp [B], g_alpha [B,N], g_acc [B], g_w [B,N]; None = absent) of one kind."""
    g = torch.Generator().manual_seed(case.seed + 77)
    B, N = case.B, case.N
    full = [torch.randn(s, generator=g) for s in ((B, 3), (B,), (B, N), (B,), (B, N))]
    if kind == "all":
        return full
    if kind == "w":
        j, _ = pick_w_samples(fw)
        onehot = torch.zeros(B, N)
        onehot[torch.arange(B), j] = 1.0
        return [None, None, None, None, onehot]
    k = NAMES.index(kind)
    return [c if i == k else None for i, c in enumerate(full)]


def loss_of(outs, coef):
    return sum((c.to(o.device, o.dtype) * o).sum() for c, o in zip(coef, outs) if c is not None)


def oracle_grad(raw, ts, d, coef, dtype):
    """d loss / d raw through oracle.volume_render's autograd in ``dtype``, as a float64 numpy array."""
    r = raw.to(dtype).clone().requires_grad_(True)
    loss_of(O.volume_render(r, ts.to(dtype), d.to(dtype)), coef).backward()
    return r.grad.double().numpy()


def model_alpha(fw, g_alpha):
    """(want [B,N,4], unit [B,N]) for g_alpha alone."""
    col = g_alpha.double() * fw["ds"]
    want = torch.zeros(*col.shape, 4, dtype=torch.float64)
    want[..., 3] = col
    return want.numpy(), (EPS * col.abs() + _subnormal_terms(col, fw["spd"])).numpy()


def model_w(fw, j):
    """(want [B,N,4], unit [B,N]) for g_w = one-hot at j[B]; unit is +inf on the elements of rays that are not judged
    and 0 where the value is a structural zero (i > j)."""
    alpha, f, T, ds = fw["alpha"], fw["f"], fw["T"], fw["ds"]
    B, N = alpha.shape
    rows = torch.arange(B)
    idx = torch.arange(N)[None, :]
    jj = j[:, None]
    wj, Tj = (alpha * T)[rows, j][:, None], T[rows, j][:, None]
    col = torch.where(idx < jj, -wj * ds / f, torch.where(idx == jj, Tj * ds, torch.zeros_like(ds)))
    common = EPS * (1 + 1 / alpha.abs().clamp_min(1e-300) + torch.cumsum(1 + 1 / f, dim=1))
    u = common[rows, j][:, None] + EPS / f
    unit = u * col.abs() + _subnormal_terms(col, fw["spd"])
    row_u = torch.where(idx <= jj, u, torch.zeros_like(u)).max(dim=1).values
    unit = torch.where((row_u > JUDGED_MAX_UNIT)[:, None], torch.full_like(unit, float("inf")), unit)
    unit = torch.where(idx > jj, torch.zeros_like(unit), unit)
    want = torch.zeros(B, N, 4, dtype=torch.float64)
    want[..., 3] = col
    return want.numpy(), unit.numpy()


def element_ratio(got, want, unit):
    """max over the judged elements of |got - want| / unit on the sigma column (0 / 0 = 0: a structural zero that is met);
    the colour columns of these two kinds are structural zeros and are checked for equality by the caller."""
    err = np.abs(np.asarray(got, dtype=np.float64)[..., 3] - want[..., 3])
    fin = np.isfinite(unit)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / unit)
    return float(r[fin].max()) if fin.any() else 0.0


def model_backward(fw, raw, ts, coef):
    """The compositor's backward in closed form, float64: (want [B,N,4], A [B,N,4]).

    With G_i = dL/dw_i gathered from every output (its terms: g_rgb . c_i, gdep t_i, gac, g_w_i; gdep and gac carry the
    disparity's slope, zero on the clamp branch), S_i = sum_{k>i} G_k w_k:
        d_raw[i, :3] = w_i g_rgb          d_raw[i, 3] = ds_i (G_i T_i - S_i / f_i + g_alpha_i)
    A is the first-order bound of what fp32 does to these, in units of EPS: every alpha_k = 1 - e_k and every factor f_k
    carries an absolute rounding of one EPS, so T_i carries the relative error kappa_i = 1 + sum_{k<i} 1/f_k and
    w_k = alpha_k T_k the absolute one T_k (1 + alpha_k kappa_k); sums are bounded by the sums of their terms' magnitudes
    (|G| -> the sum of |terms|: the disparity's two terms and acc = 1 - prod f cancel almost completely); in S_i / f_i
    the factor f_i cancels against the one inside every w_k, k > i, so it is left out of their kappa; ds_i = e_i delta_i
    softplus'_i carries (1 + x_i), x_i = softplus(sigma_i) delta_i the rounded argument of the exponential:
        A[i, c] = |g_rgb_c| T_i (1 + alpha_i kappa_i)
        A[i, 3] = |ds_i| (|G|_i T_i kappa_i + sum_{k>i} |G|_k T_k (1 + alpha_k (kappa_k - 1/f_i)) / f_i + |g_alpha_i|)
                  + |d_raw[i, 3]| (1 + x_i)  + the subnormal terms of the module docstring, in units of EPS."""
    c, t = raw[..., :3].double(), ts.double()
    B, N = t.shape
    zero = torch.zeros(B, N, dtype=torch.float64)
    g_rgb, g_disp, g_alpha, g_acc, g_w = [None if g is None else g.double() for g in coef]
    alpha, f, T, ds, w = fw["alpha"], fw["f"], fw["T"], fw["ds"], fw["w"]
    terms = []
    if g_rgb is not None:
        terms += [g_rgb[:, None, k] * c[..., k] for k in range(3)]
    if g_disp is not None:
        depth, acc = (w * t).sum(dim=1), w.sum(dim=1)
        q = depth / acc
        live = q > 1e-10                  # zero slope on the clamp branch and, the kernel's convention, on an empty ray (0/0)
        dq = torch.where(live, -g_disp / (q * q), torch.zeros_like(q))
        safe = torch.where(live, acc, torch.ones_like(acc))
        terms += [(dq / safe)[:, None] * t, (-dq * depth / (safe * safe))[:, None].expand(B, N)]
    if g_acc is not None:
        terms.append(g_acc[:, None].expand(B, N))
    if g_w is not None:
        terms.append(g_w)
    G = sum(terms, zero)
    Gabs = sum((x.abs() for x in terms), zero)

    def later(v):                                            # sum_{k>i} v_k
        rc = torch.flip(torch.cumsum(torch.flip(v, [1]), dim=1), [1])
        return torch.cat([rc[:, 1:], torch.zeros_like(rc[:, :1])], dim=1)

    ga = zero if g_alpha is None else g_alpha
    col = ds * (G * T - later(G * w) / f + ga)
    kappa = 1 + torch.cumsum(1 / f, dim=1) - 1 / f
    x = -torch.log(fw["e"].clamp_min(1e-300))
    # sum_{k>i} |G|_k T_k (1 + alpha_k (kappa_k - 1/f_i)): kappa without factor i, formed without the subtraction
    inv = (1 / f)[:, None, :].expand(B, N, N) * (1 - torch.eye(N, dtype=torch.float64))        # [b, i, m]: 1/f_m, 0 at m = i
    kappa_wo = 1 + torch.cumsum(inv, dim=2) - inv                                              # [b, i, k]
    behind = torch.triu(torch.ones(N, N, dtype=torch.float64), diagonal=1)                    # k > i
    tail = ((Gabs * T)[:, None, :] * (1 + alpha[:, None, :] * kappa_wo) * behind).sum(dim=2)
    a_col = ds.abs() * (Gabs * T * kappa + tail / f + ga.abs()) + col.abs() * (1 + x) + _subnormal_terms(col, fw["spd"]) / EPS
    want, A = torch.zeros(B, N, 4, dtype=torch.float64), torch.zeros(B, N, 4, dtype=torch.float64)
    want[..., 3], A[..., 3] = col, a_col
    if g_rgb is not None:
        want[..., :3] = w[..., None] * g_rgb[:, None, :]
        A[..., :3] = (T * (1 + alpha * kappa))[..., None] * g_rgb[:, None, :].abs()
    return want.numpy(), A.numpy()


def ray_ratios(got, want, A, keep=None):
    """Per ray, for the colour block and the sigma column ([B,2] each):
      cond  = max_i |got - want| / (EPS max_i A_i)          -- every ray
      plain = max_i |got - want| / (EPS max_i |want_i|)     -- the ray's own largest gradient as the scale; NaN where the ray
              is not JUDGED: max_i A_i > PLAIN_JUDGED max_i |want_i|, i.e. the block's largest element says little about
              its fp32 error (front samples saturated into the 2^-24 grid of 1 - alpha, or a block that is all
              cancellation, such as d acc / d sigma: acc = 1 - prod f).
    0 / 0 = 0.  keep [B,N,4]: the entries that enter the maxima (default: all)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    keep_all = np.ones(want.shape, dtype=bool) if keep is None else keep & np.isfinite(A)
    B = want.shape[0]
    cond, plain = np.zeros((B, 2)), np.zeros((B, 2))
    for c, block in enumerate((slice(0, 3), slice(3, 4))):
        k_ = keep_all[..., block].reshape(B, -1)
        flat = [np.where(k_, v[..., block].reshape(B, -1), 0.0) for v in (got, want, A)]
        err, scale, a_max = np.abs(flat[0] - flat[1]).max(axis=1), np.abs(flat[1]).max(axis=1), flat[2].max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            cond[:, c] = np.where(err == 0, 0.0, err / (EPS * a_max))
            plain[:, c] = np.where(a_max <= PLAIN_JUDGED * scale, np.where(err == 0, 0.0, err / (EPS * scale)), np.nan)
    return cond, plain


# ---- g_disp on the clamp branch and on empty rays -------------------------------------------------------------------
def disp_edge_inputs():
    """raw, ts, d, g_disp and the kind of every ray: 'clamp-' (negative positions: depth / acc < 0 <= 1e-10), 'clamp0'
    (positions below 1e-11: only the last sample has a delta, depth / acc <= 1e-11), 'empty' (every sigma -1e4 or -inf:
    acc == 0, disparity 1 / max(1e-10, 0/0) = NaN), 'plain'."""
    g = torch.Generator().manual_seed(4242)
    B, N = 24, 65
    kinds = ["clamp-", "clamp0", "empty", "plain"] * (B // 4)
    raw = torch.randn(B, N, 4, generator=g)
    raw[..., 3] = 3 * raw[..., 3] + 1.5
    ts = torch.sort(torch.rand(B, N, generator=g) * 4 + 2, dim=1).values
    for r, k in enumerate(kinds):
        if k == "clamp-":
            ts[r] = ts[r] - 8.0
        elif k == "clamp0":
            ts[r] = ts[r] * 1e-12
        elif k == "empty":
            raw[r, :, 3] = -1e4 if r % 8 < 4 else float("-inf")
    d = torch.randn(B, 3, generator=g)
    return raw, ts, d, torch.randn(B, generator=g), kinds


# ---- non-finite inputs (rgb-only upstream) ---------------------------------------------------------------------------
NONFINITE_SHAPES = ((64, 16), (32, 64), (16, 130))


def nonfinite_inputs(k):
    """tests/test_gpu_boundary.py::test_composite_special_values_like_the_reference's scatter: special sigmas and colours
    in 30 % of the samples, one coincident pair; plus g_rgb [B,3] and which rays hold no non-finite value."""
    sig_vals = torch.tensor([0.0, 1e-8, -1e-8, 1.0, -1.0, 19.9, 20.0, 20.1, -19.9, 100.0, -100.0, 1e4, -1e4, float("inf"),
                             float("-inf"), float("nan")])
    col_vals = torch.tensor([0.0, 1.0, -1.0, 0.25, 1e30, -1e30, float("inf"), float("nan")])
    B, N = NONFINITE_SHAPES[k]
    g = torch.Generator().manual_seed(3100 + k)
    raw = torch.empty(B, N, 4)
    raw[..., 3] = sig_vals[torch.randint(0, len(sig_vals), (B, N), generator=g)]
    raw[..., :3] = col_vals[torch.randint(0, len(col_vals), (B, N, 3), generator=g)]
    share = torch.where(torch.arange(B) < B // 2, 0.7, 0.995)[:, None]      # the second half of the rays: few special values
    plain = torch.rand(B, N, generator=g) < share
    raw[plain] = torch.randn(int(plain.sum()), 4, generator=g)
    ts = torch.sort(torch.rand(B, N, generator=g) * 4 + 2, dim=1).values
    ts[:, 3] = ts[:, 2]
    d = torch.randn(B, 3, generator=g)
    clean = torch.isfinite(raw).all(dim=2).all(dim=1)
    return raw, ts, d, torch.randn(B, 3, generator=g), clean


def nonfinite_keep(ref32, want):
    """The entries rule (b) judges among non-finite ones: finite in the oracle's fp32 gradient and in the float64 one."""
    return np.isfinite(ref32) & np.isfinite(want)


# --------------------------------------------------------------------------------------------------------------------
# sampler
# --------------------------------------------------------------------------------------------------------------------
PdfCase = namedtuple("PdfCase", "id Nc Nf weights edge_u seed")
PDF_SHAPES = ((3, 1), (64, 128), (66, 65), (67, 64), (130, 129), (194, 257), (256, 256))
PDF_WEIGHTS = ("rand4", "surface", "rendered", "zero")
PDF_B = 256


def pdf_cases():
    cases = [PdfCase(f"{w}-{nc}x{nf}", nc, nf, w, False, 9000 + 10 * a + b)
             for a, (nc, nf) in enumerate(PDF_SHAPES) for b, w in enumerate(PDF_WEIGHTS)]
    # forced u = 0 and 1 - 2^-24 land in the first and the last bin whatever their mass: on weights without floor bins
    cases.append(PdfCase("rand4-130x129-edge-u", 130, 129, "rand4", True, 9900))
    return cases


def pdf_inputs(case):
    """ts [B,Nc] (oracle.sample_ts), w [B,Nc], u [B,Nf] in fp32."""
    g = torch.Generator().manual_seed(case.seed)
    B, Nc, Nf = PDF_B, case.Nc, case.Nf
    ts = O.sample_ts(torch.rand(B, Nc, generator=g))
    if case.weights == "rand4":
        w = torch.rand(B, Nc, generator=g) ** 4
    elif case.weights == "surface":
        w = torch.zeros(B, Nc)
        k = torch.randint(0, Nc, (B,), generator=g)
        side = torch.randint(0, 2, (B,), generator=g) * 2 - 1
        rows = torch.arange(B)
        w[rows, (k + side).clamp(0, Nc - 1)] = 0.05 * torch.rand(B, generator=g)
        w[rows, k] = 0.1 + 0.9 * torch.rand(B, generator=g)
    elif case.weights == "rendered":
        raw = torch.randn(B, Nc, 4, generator=g)
        raw[..., 3] *= 6.0
        d = torch.randn(B, 3, generator=g)
        w = O.volume_render(raw, ts, d / torch.norm(d, dim=1, keepdim=True))[4]
    else:
        w = torch.zeros(B, Nc)
    u = torch.rand(B, Nf, generator=g)
    if case.edge_u:
        u[::4, 5] = 0.0
        u[2::8, 70] = 1.0 - EPS                              # 1 in 8: where the last bin is under the switch this is a kink
        u[1::16, 100] = 0.0
        u[:, 17] = u[:, 90]                                  # a duplicated pair per ray
    return ts, w.contiguous(), u


def kink_window(Nc):
    """Roundings of size EPS c1 that separate the fp32 difference of two neighbouring cdf values from the float64 one: a
    sequential cumsum spends one on it, the kernel's scan at most 6 (its shuffle tree) + Nc/64 (its chunk carries) + 2
    (the two divisions by the total).  Nc roundings, the bound for an arbitrary summation order, would flag every
    floor bin (weight 0: pdf = 1e-5 / (sum w + Nc 1e-5)) of every opaque ray, whose sum w is 1."""
    return 8 + Nc / 64


def kink_cap(case):
    """The share of a case's rays that may carry a kink.  2 %, except on weights with exact floor bins next to sum w = 1
    ('surface', 'rendered'): there a floor bin's pdf sits 0.1 ... 0.3 % under the switch, well inside one rounding of
    c1, and each of the Nf samples lands in one of the ~Nc/2 floor bins with probability ~Nc/2 x 1e-5."""
    return max(KINK_CAP, case.Nf * case.Nc * 0.5e-5) if case.weights in ("surface", "rendered") else KINK_CAP


def model_pdf(ts, w, u):
    """oracle.sample_pdf in float64, opened up: (sorted positions [B,Nc+Nf], the ray's unit [B], kink [B])."""
    ts, w, u = ts.double(), w.double(), u.double()
    Nc = ts.shape[1]
    bins = 0.5 * (ts[:, 1:] + ts[:, :-1])
    wt = w[:, 1:-1] + 1e-5
    pdf = wt / torch.sum(wt, -1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)
    inds = torch.searchsorted(cdf, u.contiguous(), right=True)
    below = torch.clamp(inds - 1, min=0)
    above = torch.clamp(inds, max=cdf.shape[-1] - 1)
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    b0, b1 = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    raw_denom = c1 - c0
    denom = torch.where(raw_denom < 1e-5, torch.ones_like(raw_denom), raw_denom)
    z = b0 + (u - c0) / denom * (b1 - b0)
    unit = EPS * ((b1 - b0) * (1 + (c1 + u) / denom) + z.abs())
    win = kink_window(Nc) * EPS * c1 + EPS * 1e-5
    kink = (raw_denom - 1e-5).abs() <= win
    # a bin under the switch maps all of its u to b0 (+ at most 1e-5 of its width) and the next bin starts at b1: z jumps
    # at its upper edge, so a u within the cdf's rounding of that edge, from either side, is a kink as well
    below_mass = c0 - torch.gather(cdf, 1, torch.clamp(below - 1, min=0))
    kink |= (raw_denom < 1e-5) & (above > below) & (c1 - u <= win)
    kink |= (below >= 1) & (below_mass < 1e-5) & (u - c0 <= win)
    return torch.sort(torch.cat([ts, z], -1), -1).values.numpy(), unit.max(dim=1).values.numpy(), kink.any(dim=1).numpy()


def pdf_ratios(got, want, unit):
    """[B]: sup norm of the difference of the SORTED rows, in the ray's unit."""
    got = np.sort(np.asarray(got, dtype=np.float64), axis=1)
    return np.abs(got - want).max(axis=1) / unit


# --------------------------------------------------------------------------------------------------------------------
# the reference's own error in these units: what the constants above record
# --------------------------------------------------------------------------------------------------------------------
def measure():
    c_alpha = {k: 0.0 for k in C_REF_ALPHA}
    c_alpha_cond = c_w_cond = 0.0
    c_w = {k: 0.0 for k in C_REF_W}
    c_ray = {k: 0.0 for k in C_REF_RAY}
    c_plain = {k: 0.0 for k in C_REF_RAY}
    n_plain = {k: np.zeros(2, dtype=np.int64) for k in C_REF_RAY}
    judged_share = {}
    for case in comp_cases():
        raw, ts, d = comp_inputs(case)
        fw = forward64(raw, ts, d)
        g = coefs(case, "alpha")
        want, unit = model_alpha(fw, g[2])
        ref32 = oracle_grad(raw, ts, d, g, torch.float32)
        c_alpha[case.set] = max(c_alpha[case.set], element_ratio(ref32, want, unit))
        c_alpha_cond = max(c_alpha_cond, element_ratio(ref32, want, EPS * model_backward(fw, raw, ts, g)[1][..., 3]))
        j, judged = pick_w_samples(fw)
        judged_share[case.id] = float(judged.float().mean())
        want, unit = model_w(fw, j)
        g = coefs(case, "w", fw)
        ref32 = oracle_grad(raw, ts, d, g, torch.float32)
        c_w[case.set] = max(c_w[case.set], element_ratio(ref32, want, unit))
        c_w_cond = max(c_w_cond, element_ratio(ref32, want, EPS * model_backward(fw, raw, ts, g)[1][..., 3]))
        for kind in c_ray:
            g = coefs(case, kind)
            want, A = model_backward(fw, raw, ts, g)
            ref32 = oracle_grad(raw, ts, d, g, torch.float32)
            cond, plain = ray_ratios(ref32, want, A, np.isfinite(ref32))
            c_ray[kind] = max(c_ray[kind], float(cond.max()))
            c_plain[kind] = max(c_plain[kind], float(np.nanmax(plain, initial=0.0)))
            n_plain[kind] += np.array([np.isfinite(plain).sum(), plain.size])
    c_nf = 0.0
    for k in range(len(NONFINITE_SHAPES)):
        raw, ts, d, g_rgb, _ = nonfinite_inputs(k)
        g = [g_rgb, None, None, None, None]
        ref32, want = oracle_grad(raw, ts, d, g, torch.float32), oracle_grad(raw, ts, d, g, torch.float64)
        with np.errstate(all="ignore"):
            A = model_backward(forward64(raw, ts, d), raw, ts, g)[1]
        c_nf = max(c_nf, float(ray_ratios(ref32, want, A, nonfinite_keep(ref32, want))[0].max()))
    c_pdf, kinks = 0.0, {}
    for case in pdf_cases():
        ts, w, u = pdf_inputs(case)
        want, unit, kink = model_pdf(ts, w, u)
        r = pdf_ratios(O.sample_pdf(ts, w, u).numpy(), want, unit)
        kinks[case.id] = int(kink.sum())
        c_pdf = max(c_pdf, float(r[~kink].max()))
    return dict(C_REF_ALPHA=c_alpha, C_REF_ALPHA_COND=c_alpha_cond, C_REF_W=c_w, C_REF_W_COND=c_w_cond, C_REF_RAY=c_ray, C_REF_RAY_PLAIN=c_plain,
                plain_judged={k: tuple(int(x) for x in v) for k, v in n_plain.items()}, C_REF_NONFINITE=c_nf, C_REF_PDF=c_pdf,
                judged_share=judged_share, kinks=kinks)


if __name__ == "__main__":
    m = measure()
    for k in ("C_REF_ALPHA", "C_REF_ALPHA_COND", "C_REF_W", "C_REF_W_COND", "C_REF_RAY", "C_REF_RAY_PLAIN", "plain_judged", "C_REF_NONFINITE", "C_REF_PDF"):
        print(k, "=", m[k])
    print("smallest judged share of a 'w' case:", min(m["judged_share"].items(), key=lambda kv: kv[1]))
    print("most kink rays of a sampler case:", max(m["kinks"].items(), key=lambda kv: kv[1]))
