"""Adam's step as the library's kernels take it (csrc/adam.hip ``adam_element``; include/nerf_amd.h nerf_amd_adam_step), in
numpy float64, with a bound per element derived from the kernel's operation count -- for the tests to hold the three Adam
kernels and the graphed steppers' per-step scalars to.

The scalars
-----------
``scalars(lr, betas, eps, t)`` is the header's rule: the betas are rounded to fp32 (what the kernel multiplies by), the bias
corrections are formed in double from those rounded betas,

    bc1 = fl32(1 - b1f**t)            bc2s = fl32(sqrt(1 - b2f**t))

and lr and eps are rounded to fp32.  Every Adam launch of the library must run with exactly these six numbers.

The element
-----------
``adam_element`` is, with every value an fp32 number and fl() one rounding to nearest:

    mi    = b1 m + (1 - b1) g                    three or two roundings: the compiler may fuse either product into the sum
    vi    = b2 v + ((1 - b2) g) g                four or three roundings, likewise
    denom = sqrtf(vi) / bc2s + eps               sqrtf, a division, a sum
    p    -= (lr / bc1) (mi / denom)              two divisions, a product (fused into the difference, or not), the difference

``1 - b`` is one fp32 subtraction of two fp32 numbers and ``lr / bc1`` one fp32 division of two: no choice is open to the
compiler there, the model forms them the same way (``omb1``, ``omb2``, ``a``) and takes them as exact operands.  Everything
else is evaluated in float64 on those fp32 operands: M, V, S = sqrt(V), Q = S / bc2s, D = Q + eps, R = M / D, P = p - a R.

The flags
---------
csrc/Makefile compiles with ``-O3 -std=c++20 --offload-arch=gfx950`` and nothing that touches floating point: no
-ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt, no flush-to-zero flag.  hipcc's defaults therefore hold:
  * fp32 division and ``sqrtf`` are CORRECTLY ROUNDED (half an ulp: the v_div_scale / v_div_fmas / v_div_fixup sequence and
    v_sqrt_f32 with its correction steps are in the kernels' code; the kernel descriptors say denorm mode 3, round mode 0);
  * -ffp-contract=fast: an ``a * b + c`` may become one fma, with one rounding instead of two, in either of its products;
  * fp32 subnormals are kept, not flushed.
So every operation above errs by at most u = 2^-24 of its result (half an ulp), or by eta = 2^-150 (half the smallest
subnormal) where the result is subnormal, and the bound below allows BOTH spellings of each a * b + c: it charges the
product's rounding as if unfused (a fused one errs less) and the sum's rounding on the result.

The bounds (no measured constant: u, eta and the operation count)
------------------------------------------------------------------
Write |x| for magnitudes of the float64 model's values.

  m:  the two products err by u |b1 m| and u |omb1 g|, the sum by u of what it holds:
        E_m = u (|b1 m| + |omb1 g|) (1 + u) + u |M| + 3 eta
  v:  w = fl(omb2 g) errs by u |w|, carried into w g; that product errs by u again; b2 v by u |b2 v|; the sum by u:
        E_v = u (|b2 v| + 2 |omb2 g^2|) (1 + 2 u) + u |V| + eta (|g| + 3)
      (eta |g|: a subnormal w's rounding, multiplied by g.)
  S:  |sqrt(V') - sqrt(V)| = |V' - V| / (sqrt(V') + sqrt(V)) <= min(E_v / S, sqrt(E_v))    (the second form where V is 0 or
      tiny: a square that underflowed), then sqrtf's own half ulp:
        E_s = e + u (S + e),   e = min(E_v / S, sqrt(E_v))
  Q:    E_q = E_s / bc2s + u (Q + E_s / bc2s) + eta
  D:    E_d = E_q + u (D + E_q)
  R:  m'/d' - M/D = ((m' - M) D - M (d' - D)) / (d' D), and d' >= D - E_d > 0 (asserted):
        E_r = f + u (|R| + f) + eta,   f = (E_m + |R| E_d) / (D - E_d)
  P:  the product a r errs by a E_r and, where it is not fused, by its own rounding; the difference rounds once:
        e' = a E_r + u (a |R| + a E_r) + eta
        E_p = e' + u (|P| + e') + eta
Each bound is multiplied by 1 + 2^-20 for the terms of second order left out and for the float64 evaluation of the model
itself (fewer than 32 operations of 2^-53 each: below 2^-29 of the fp32 term beside it).

Where fp32 leaves its range
---------------------------
V >= 2^128 - 2^103 (what rounds to +inf in fp32; with v >= 0 the sum overflows in every spelling as soon as its product does):
the model states v = +inf, and then sqrtf = inf, denom = inf, mi / denom = 0, the update a * 0 = 0: p keeps its value.  The
bounds of v and p are 0 there -- equality.  An element whose V lies within E_v of that threshold is ``ambiguous`` (fused and
unfused spellings may differ): the tests plant none and assert there is none.  A square that underflows ((1 - b2) g^2 below
2^-150: |g| = 1e-23) needs no case of its own: eta and the sqrt(E_v) branch carry it.
"""
import math
from collections import namedtuple

import numpy as np

F32 = np.float32
U = 2.0 ** -24                    # half an ulp of fp32, relative
ETA = 2.0 ** -150                 # half the smallest fp32 subnormal
SLACK = 1.0 + 2.0 ** -20          # second-order terms and the float64 evaluation (module docstring)
INF_FROM = 2.0 ** 128 - 2.0 ** 103      # the smallest real number that rounds to +inf in fp32

Result = namedtuple("Result", "p m v bp bm bv v_inf ambiguous")


def f32(x):
    """``x`` rounded to fp32, as a Python float."""
    return float(F32(x))


def scalars(lr, betas, eps, t):
    """{lr, b1, b2, eps, 1 - b1^t, sqrt(1 - b2^t)} as fp32[6] by the rule of include/nerf_amd.h nerf_amd_adam_step."""
    b1, b2, t = f32(betas[0]), f32(betas[1]), int(t)
    bc1 = 1.0 - b1 ** t
    bc2s = math.sqrt(1.0 - b2 ** t)
    return np.array([float(lr), b1, b2, float(eps), bc1, bc2s], dtype=np.float32)


def hyper_words(s, t):
    """The 8 words of a ring slot / of ``stepper.hyper`` as int32[8]: the six scalars' bits and ``t`` as an int64."""
    out = np.zeros(8, dtype=np.int32)
    out[:6] = np.asarray(s, dtype=np.float32).view(np.int32)
    out[6:8] = np.array([int(t)], dtype=np.int64).view(np.int32)
    return out


def element64(p, m, v, g, b1, b2, eps, bc2s, omb1, omb2, a):
    """The element update in float64 on whatever operands are given (no rounding anywhere) and the bounds of the module
    docstring for an fp32 kernel on the same operands: (P, M, V, E_p, E_m, E_v, v_inf, ambiguous)."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        t1, t2 = b1 * m, omb1 * g
        M = t1 + t2
        em = U * (np.abs(t1) + np.abs(t2)) * (1 + U) + U * np.abs(M) + 3 * ETA
        t3, t4 = (omb2 * g) * g, b2 * v
        V = t4 + t3
        ev = U * (np.abs(t4) + 2 * np.abs(t3)) * (1 + 2 * U) + U * np.abs(V) + ETA * (np.abs(g) + 3)
        v_inf = V >= INF_FROM
        ambiguous = np.isfinite(V) & ((V + ev >= INF_FROM) != (V - ev >= INF_FROM))
        S = np.sqrt(V)
        e = np.where(S > 0, np.minimum(ev / np.where(S > 0, S, 1.0), np.sqrt(ev)), np.sqrt(ev))
        es = e + U * (S + e)
        Q = S / bc2s
        eq = es / bc2s + U * (Q + es / bc2s) + ETA
        D = Q + eps
        ed = eq + U * (D + eq)
        fin = ~v_inf
        if not bool(np.all(D[fin] - ed[fin] > 0)):
            raise ValueError("the model needs denom - its error > 0 (eps > 0)")
        R = M / D
        f = (em + np.abs(R) * ed) / (D - ed)
        er = f + U * (np.abs(R) + f) + ETA
        P = p - a * R
        e1 = a * er + U * (a * np.abs(R) + a * er) + ETA
        ep = e1 + U * (np.abs(P) + e1) + ETA
        # fp32 leaves its range: v = +inf, the update is a * (m / inf) = 0 and p keeps its value -- equalities
        V = np.where(v_inf, np.inf, V)
        P = np.where(v_inf, p, P)
        ev = np.where(v_inf, 0.0, ev * SLACK)
        ep = np.where(v_inf, 0.0, ep * SLACK)
    return P, M, V, ep, em * SLACK, ev, v_inf, ambiguous


def step(p, m, v, g, s):
    """One step on fp32 operands ``p, m, v, g`` (arrays) with the fp32 scalars ``s`` = ``scalars(...)``: a Result of float64
    model values, bounds, the elements whose v is +inf and the ambiguous ones.  v must not be negative."""
    p, m, v, g = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (p, m, v, g))
    s = np.asarray(s, dtype=np.float32)
    lr, b1, b2, eps, bc1, bc2s = (F32(x) for x in s[:6])
    if not bool(np.all(v >= 0)):
        raise ValueError("the second moment is never negative")
    omb1, omb2 = F32(1) - b1, F32(1) - b2                 # the kernel's fp32 subtractions
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        a = lr / bc1                                      # the kernel's fp32 division
    out = element64(p, m, v, g, float(b1), float(b2), float(eps), float(bc2s), float(omb1), float(omb2), float(a))
    if not bool(np.all(np.isfinite(out[1]))) or float(np.max(np.abs(out[1]), initial=0.0)) >= INF_FROM:
        raise ValueError("the first moment leaves fp32: not a case of this model")
    return Result(*out)


def ratios(res, p, m, v):
    """The worst |got - model| / bound of each output over all elements, as {"p":, "m":, "v":} -- 0 where a bound of 0 is met
    exactly, inf where it is not (or where a value that must be +inf is not)."""
    out = {}
    for name, got, want, bound in (("p", p, res.p, res.bp), ("m", m, res.m, res.bm), ("v", v, res.v, res.bv)):
        got = np.asarray(got, dtype=np.float32).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            same = got == want                             # covers +inf == +inf
            err = np.where(same, 0.0, np.abs(got - want))
            r = np.where(same, 0.0, np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.inf))
        r = np.where(np.isnan(r), np.inf, r)
        out[name] = float(np.max(r, initial=0.0))
    return out


# ---- fp32 emulations of the kernel's two extreme spellings, for the CPU self-checks ------------------------------------------
def _fma(a, b, c):
    """fl32(a b + c) for fp32 arrays: the product of two fp32 numbers is exact in float64; the float64 sum's own rounding is
    2^-29 of an fp32 ulp."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate(p, m, v, g, s, fused):
    """``adam_element`` in numpy fp32, every a * b + c unfused (``fused=False``) or fused (``True``: the second product of
    each sum).  numpy's fp32 division and sqrt are correctly rounded, as the kernel's are."""
    p, m, v, g = (np.asarray(x, dtype=np.float32) for x in (p, m, v, g))
    lr, b1, b2, eps, bc1, bc2s = (F32(x) for x in np.asarray(s, dtype=np.float32)[:6])
    one = F32(1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        if fused:
            mi = _fma(np.full_like(g, one - b1), g, b1 * m)
            vi = _fma((one - b2) * g, g, b2 * v)
        else:
            mi = b1 * m + (one - b1) * g
            vi = b2 * v + (one - b2) * g * g
        denom = np.sqrt(vi) / bc2s + eps
        r = mi / denom
        a = lr / bc1
        pn = _fma(np.full_like(r, -a), r, p) if fused else p - a * r
    return pn, mi, vi
