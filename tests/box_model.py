"""The scene box's placement (include/nerf_amd.h "scene box", csrc/ray_box_device.h) restated in torch on the CPU: op for op in
fp32 -- what nerf_amd_box_positions must equal bit for bit -- and once more in float64, with the distance allowed between the
two DERIVED from the operation count below.  Nothing here is taken from what a GPU shows.

Definition, per ray (o, d) and box lo < hi, interval tn < tf (every fp32 operation rounded on its own, no fma):
    per axis a with d_a != 0:  ta = (lo_a - o_a) / d_a, tb = (hi_a - o_a) / d_a, near = min(ta, tb), far = max(ta, tb)
             a with d_a == 0:  nothing if lo_a <= o_a <= hi_a, else the ray misses
    t0 = max(tn, near_x, near_y, near_z), t1 = min(tf, far_x, far_y, far_z), folded in that order
    hit = inside and (t0 < t1)  (false for a NaN);  a miss: t0 = tn, t1 = tf
    c_i = h u_i + b_i on the unit bins b = linspace(0, 1, N + 1), h = b_1 - b_0  (or given)
    ts_i = min(t0 + (t1 - t0) c_i, t1)
min / max are comparisons that let a NaN of either side through:  max(a, b) = a if (a > b or a != a) else b.

The bound (EPS = 2^-24, the unit roundoff of fp32; T = max(|tn|, |tf|), D = tf - tn; a ray on which both models agree
about `hit`):
  * ta = fl(fl(lo - o) / d): one subtraction, one division -> |ta - ta*| <= 2 EPS |ta*| (1 + EPS).
  * the min / max chain selects, it does not round.  Let j be the fp32 arg max and k the exact one: t0 - t0* = a_j - a_k* lies
    between a_k - a_k* >= -2 EPS |t0*| and a_j - a_j* <= 2 EPS |a_j*|, and a hit has tn <= t0 < t1 <= tf, so
    |t0 - t0*| <= 2 EPS T and likewise |t1 - t1*| <= 2 EPS T (tn and tf themselves are exact).
  * c = fl(fl(h u) + b): two roundings -> |c - c*| <= 2 EPS cm, cm = max(1, |c*|); given unit positions: exact.
  * ts: three roundings.  L = t1 - t0: |L - L*| <= 4 EPS T before its own rounding; p = fl(fl(L) c):
    |p - L* c*| <= |L - L*| cm + |L*| |c - c*| + 2 EPS |L| cm <= (4 T + 2 D + 2 D) EPS cm; v = fl(t0 + p):
    |v - v*| <= 2 EPS T + (4 T + 4 D) EPS cm + EPS T (unit positions lie in [0, 1], so |v| <= T);  min(v, t1) is
    1-Lipschitz in both arguments, and t1's own 2 EPS T is the smaller of the two.
    =>  |ts - ts*| <= EPS (7 T + 4 D) cm, times (1 + 2^-10) for the second-order terms dropped above; with given unit
    positions the |L*| |c - c*| term is gone: EPS (7 T + 2 D) cm.
For tn = 2, tf = 6 that is 58 EPS = 3.5e-6 at cm = 1.
A ray on which the two models DISAGREE about `hit` must be a grazing one: |t1* - t0*| <= 4 EPS T (``agree_or_grazing``).
"""
import numpy as np
import torch

EPS = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10

# the table's box and interval: not symmetric, no face through the origin, every bound exact in fp32
LO, HI, TN, TF = (-1.0, -0.75, -1.25), (1.0, 0.5, 0.75), 2.0, 6.0

CLASSES = ("through", "origin_inside", "nearer_than_tn", "beyond_tf", "sideways", "zero_plus_inside", "zero_minus_inside",
           "zero_plus_outside", "zero_minus_outside", "negative_direction", "along_face", "nan_origin", "nan_direction",
           "clipped_tn_only", "clipped_tf_only", "clipped_neither")


def _max(a, b):
    return torch.where((a > b) | torch.isnan(a), a, b)


def _min(a, b):
    return torch.where((a < b) | torch.isnan(a), a, b)


def span(rays, lo, hi, tn, tf):
    """(t0 [B], t1 [B], hit [B] bool) in the dtype of ``rays`` (float32: the kernel's operations one by one; float64: the
    same formula)."""
    dt = rays.dtype
    B = rays.shape[0]
    t0, t1 = torch.full((B,), tn, dtype=dt), torch.full((B,), tf, dtype=dt)
    inside = torch.ones(B, dtype=torch.bool)
    for a in range(3):
        o, d = rays[:, a], rays[:, 3 + a]
        lo_a, hi_a = torch.tensor(lo[a], dtype=dt), torch.tensor(hi[a], dtype=dt)
        nz = d != 0                                   # true for a NaN d
        dd = torch.where(nz, d, torch.ones_like(d))   # the quotient of a zero d is not looked at
        ta, tb = (lo_a - o) / dd, (hi_a - o) / dd
        t0 = torch.where(nz, _max(t0, _min(ta, tb)), t0)
        t1 = torch.where(nz, _min(t1, _max(ta, tb)), t1)
        inside &= nz | ((o >= lo_a) & (o <= hi_a))
    hit = inside & (t0 < t1)
    return (torch.where(hit, t0, torch.full_like(t0, tn)), torch.where(hit, t1, torch.full_like(t1, tf)), hit)


def unit_bins(N):
    """The bins the placement jitters in, as the package forms them."""
    return torch.linspace(0, 1, N + 1)


def unit_positions(u, N, dtype=torch.float32):
    """c [B, N] of explicit uniforms u [B, N] (fp32 values): h u + b_i on the fp32 unit bins, in ``dtype``."""
    b = unit_bins(N)
    h = (b[1] - b[0]).to(dtype)                       # b_0 = 0: the difference is exact
    return h * u.to(dtype) + b[:N].to(dtype)


def place(t0, t1, c):
    """ts [B, N] = min(t0 + (t1 - t0) c, t1), each operation on its own."""
    v = t0[:, None] + (t1 - t0)[:, None] * c
    return torch.where(v < t1[:, None], v, t1[:, None].expand_as(v))


def positions(rays, lo, hi, tn, tf, c):
    """(ts [B,N], span [B,2], hit [B] int32) for unit positions c [B,N], in the dtype of ``rays`` and ``c``."""
    t0, t1, hit = span(rays, lo, hi, tn, tf)
    return place(t0, t1, c), torch.stack([t0, t1], dim=1), hit.to(torch.int32)


def bound(c64, tn, tf, given=False):
    """The derived |ts - ts*| allowance per element (module docstring); ``given``: c carries no rounding of its own."""
    T, D = max(abs(tn), abs(tf)), tf - tn
    cm = torch.clamp(c64.abs(), min=1.0)
    return EPS * (7.0 * T + (2.0 if given else 4.0) * D) * cm * SLACK


def agree_or_grazing(hit32, rays64, lo, hi, tn, tf):
    """Every ray on which the fp32 and the float64 model disagree about `hit` is a grazing one."""
    bad = hit32.bool() != span(rays64, lo, hi, tn, tf)[2]
    if not bool(bad.any()):
        return True
    # a miss reports (tn, tf): look at the un-replaced interval of the rays in question
    t0r, t1r = _raw_span64(rays64[bad], lo, hi, tn, tf)
    return bool(((t1r - t0r).abs() <= 4 * EPS * max(abs(tn), abs(tf))).all())


def _raw_span64(rays, lo, hi, tn, tf):
    """(t0, t1) of the slab chain alone, before the hit test replaces a miss by (tn, tf)"""
    t0, t1 = torch.full((rays.shape[0],), tn, dtype=torch.float64), torch.full((rays.shape[0],), tf, dtype=torch.float64)
    for a in range(3):
        o, d = rays[:, a], rays[:, 3 + a]
        nz = d != 0
        dd = torch.where(nz, d, torch.ones_like(d))
        ta, tb = (lo[a] - o) / dd, (hi[a] - o) / dd
        t0 = torch.where(nz, _max(t0, _min(ta, tb)), t0)
        t1 = torch.where(nz, _min(t1, _max(ta, tb)), t1)
    return t0, t1


# ---- the case table -------------------------------------------------------------------------------------------------------
def _aim(origin, target, scale=1.0):
    o, t = np.asarray(origin, np.float64), np.asarray(target, np.float64)
    d = (t - o) / np.linalg.norm(t - o) * scale
    return [*o, *d]


def case_table(B, seed=0):
    """rays [B, 6] float32 and, per ray, the name of the class it was BUILT for (``classify`` checks each against the float64
    model).  The first rows are one ray per class of CLASSES (B >= 32); the rest are random rays from a radius-4 sphere
    aimed at random points in and around the box."""
    nan, z = float("nan"), 0.0
    rows = [
        ("through", _aim((0.0, 0.0, 4.0), (0.2, -0.1, 0.0))),                       # enters at ~3.25, leaves at ~5.25
        ("clipped_neither", _aim((3.0, 2.0, -1.5), (0.1, -0.2, -0.3))),
        ("origin_inside", _aim((0.1, -0.2, 0.3), (4.0, 1.0, 2.0), 0.3)),            # near < 0 < tn, far ~ 3.2
        ("clipped_tn_only", _aim((0.5, 0.2, -0.4), (-3.0, -4.0, 1.0), 0.25)),       # origin inside, far in (tn, tf)
        ("clipped_tf_only", _aim((0.0, 0.0, 4.0), (0.1, 0.1, 0.0), 0.6)),           # enters at ~5.4, leaves at ~8.8
        ("origin_inside", _aim((0.0, -0.1, -0.2), (1.0, 0.3, 0.2), 0.1)),           # far > tf as well: [tn, tf], a hit
        ("nearer_than_tn", _aim((0.0, 0.0, 2.0), (0.0, 0.05, 0.0), 2.0)),           # leaves at ~1.6 < tn
        ("beyond_tf", _aim((0.0, 4.0, 0.0), (0.1, 0.0, 0.1), 0.25)),                # enters at ~14 > tf
        ("sideways", _aim((0.0, 0.0, 4.0), (3.0, 0.5, 3.5))),
        ("sideways", _aim((4.0, 0.0, 0.0), (3.5, 2.0, 1.0))),
        ("zero_plus_inside", [0.25, 0.1, 4.0, z, 0.02, -1.0]),
        ("zero_minus_inside", [0.25, 0.1, 4.0, -z, 0.02, -1.0]),
        ("zero_plus_outside", [2.0, 0.1, 4.0, z, 0.02, -1.0]),
        ("zero_minus_outside", [2.0, 0.1, 4.0, -z, 0.02, -1.0]),
        ("zero_minus_inside", [0.25, 4.0, 0.1, 0.01, -1.0, -z]),
        ("zero_plus_outside", [0.25, 4.0, -2.0, 0.01, -1.0, z]),
        ("negative_direction", _aim((3.0, 2.5, 1.5), (0.3, 0.2, 0.1))),             # every component negative
        ("negative_direction", _aim((2.0, 2.0, 3.0), (-0.5, -0.5, -1.0))),
        ("along_face", [LO[0], 0.1, 4.0, z, z, -1.0]),                              # in the plane x = lo_x: inside by <=
        ("along_face", [0.3, HI[1], -4.0, z, -z, 1.0]),                             # in the plane y = hi_y
        ("nan_origin", [nan, 0.0, 4.0, 0.0, 0.0, -1.0]),
        ("nan_origin", [0.0, nan, 4.0, z, z, -1.0]),                                # a NaN origin on an axis with d = 0
        ("nan_direction", [0.0, 0.0, 4.0, nan, 0.0, -1.0]),
        ("nan_direction", [0.0, 0.0, 4.0, 0.0, 0.0, nan]),
    ]
    if B < len(rows):
        raise ValueError(f"the case table needs B >= {len(rows)}")
    rng = np.random.default_rng(seed)
    names, rays = [n for n, _ in rows], [r for _, r in rows]
    for _ in range(B - len(rows)):
        v = rng.normal(size=3)
        o = 4.0 * v / np.linalg.norm(v)
        target = rng.uniform(-1.6, 1.6, size=3)
        rays.append(_aim(o, target, rng.choice([1.0, 1.0, 0.7, 1.4])))
        names.append("random")
    return torch.tensor(np.asarray(rays, np.float64), dtype=torch.float32), names


def classify(rays, lo=LO, hi=HI, tn=TN, tf=TF):
    """{class name: bool mask [B]} from the float64 model and the rays' own components."""
    r = rays.double()
    _, _, hit = span(r, lo, hi, tn, tf)
    o, d = r[:, :3], r[:, 3:]
    lo_t, hi_t = torch.tensor(lo, dtype=torch.float64), torch.tensor(hi, dtype=torch.float64)
    in_slab = (o >= lo_t) & (o <= hi_t)
    zero = d == 0
    plus, minus = zero & ~torch.signbit(d), zero & torch.signbit(d)
    finite = torch.isfinite(r).all(dim=1)
    # the un-clipped crossing interval [n, f] of the slabs alone (tn = -inf, tf = +inf)
    n, f = _raw_span64(r, lo, hi, float("-inf"), float("inf"))
    slabs_ok = finite & (~zero | in_slab).all(dim=1) & (n < f)
    return {
        "through": hit & (n > tn) & (f < tf),
        "origin_inside": hit & in_slab.all(dim=1) & (n < tn),
        "nearer_than_tn": slabs_ok & (f <= tn) & (f > 0) & ~hit,
        "beyond_tf": slabs_ok & (n >= tf) & ~hit,
        "sideways": finite & ~zero.any(dim=1) & ~(n < f) & ~hit,
        "zero_plus_inside": hit & (plus & in_slab).any(dim=1),
        "zero_minus_inside": hit & (minus & in_slab).any(dim=1),
        "zero_plus_outside": finite & (plus & ~in_slab).any(dim=1) & ~hit,
        "zero_minus_outside": finite & (minus & ~in_slab).any(dim=1) & ~hit,
        "negative_direction": hit & (d < 0).all(dim=1),
        "along_face": hit & (zero & ((o == lo_t) | (o == hi_t))).any(dim=1),
        "nan_origin": torch.isnan(o).any(dim=1) & ~hit,
        "nan_direction": torch.isnan(d).any(dim=1) & ~hit,
        "clipped_tn_only": hit & (n < tn) & (f < tf),
        "clipped_tf_only": hit & (n > tn) & (f > tf),
        "clipped_neither": hit & (n > tn) & (f < tf),
    }
