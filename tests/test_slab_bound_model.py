"""A numpy MODEL of the packet walks' fused slab predicates (csrc/rtg_isect.hpp: SlabFma,
box_pass_t / box_pass_v, slab_cons_v).  It models the device code and does not run it: the
constants below are copied from the header, the arithmetic is restated in float32 with the FMA
emulated through float64 (the product of two floats is exact there), and the reciprocal is the
correctly rounded 1/d moved one ulp either way, so up to 1.5 ulp off -- beyond v_rcp_f32's 1 ulp.

Checked on seeded random box / ray pairs:
  1. a sure decision of the fused form is the division form's (box_hit's) decision;
  2. every box the division form keeps, the conservative test keeps;
  3. the sure set is not empty: at least 30 % of the pairs at 1 and 10^2 units.
"""
import numpy as np
import pytest

F = np.float32
N = 1_000_000

# --- constants of csrc/rtg_isect.hpp
REL_SLACK = F(2.0 ** -20)        # box_pass_t: relative slack of the exact decisions
ABS_SLACK = F(2.0 ** -21)        # slab_slack0: slack0 = 1e-30 + 2^-21 A
TINY = F(1e-30)
CONS_BIAS = F(2.0 ** -22)        # slab_cons_ray: e_k = 2^-22 |o_k inv_k|, per axis
CONS_REL = F(2.0 ** -20)         # slab_cons_v: 1 - 2^-20, minTc = minT (1 + 2^-20)
FAST_LO, FAST_HI = F(2.0 ** -60), F(2.0 ** 60)


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def fmin(a, b):   # fminf / fmaxf: NaN-ignoring
    return np.fmin(a, b)


def fmax(a, b):
    return np.fmax(a, b)


def box_hit(lo, hi, o, d, minT):
    """BoundingBox::doesIntersectWith as box_hit restates it: true divisions, the x slab by
    comparison, y / z by fmin / fmax."""
    with np.errstate(all="ignore"):
        t1 = (lo - o) / d
        t2 = (hi - o) / d
        swap = t1[:, 0] > t2[:, 0]
        tmin = np.where(swap, t2[:, 0], t1[:, 0])
        tmax = np.where(swap, t1[:, 0], t2[:, 0])
        for k in (1, 2):
            tmin = fmax(tmin, fmin(t1[:, k], t2[:, k]))
            tmax = fmin(tmax, fmax(t1[:, k], t2[:, k]))
        return (tmax > 0) & (tmax >= tmin) & (tmin < minT)


def fused(lo, hi, o, inv):
    """SlabFma + the six fused distances -> (tmin, tmax, A)."""
    with np.errstate(all="ignore"):
        p = o * inv
        n = -p
        A = np.max(np.abs(p), axis=1)
        t1 = fma(lo, inv, n)
        t2 = fma(hi, inv, n)
        tmin = fmax(fmax(fmin(t1[:, 0], t2[:, 0]), fmin(t1[:, 1], t2[:, 1])), fmin(t1[:, 2], t2[:, 2]))
        tmax = fmin(fmin(fmax(t1[:, 0], t2[:, 0]), fmax(t1[:, 1], t2[:, 1])), fmax(t1[:, 2], t2[:, 2]))
    return tmin, tmax, A


def box_pass(lo, hi, o, d, inv, minT):
    """box_pass_t: (sure, answer of the fast values)."""
    tmin, tmax, A = fused(lo, hi, o, inv)
    ad = np.abs(d)
    fast = np.all((ad >= FAST_LO) & (ad <= FAST_HI), axis=1)
    with np.errstate(all="ignore"):
        slack0 = np.where(fast, fma(np.full_like(A, ABS_SLACK), A, np.full_like(A, TINY)), F(np.inf)).astype(F)
        atmin, atmax = np.abs(tmin), np.abs(tmax)
        d1 = tmax - tmin
        d2 = (minT - tmin).astype(F)
        rel = np.full_like(A, REL_SLACK)
        s1 = np.abs(d1) - fma(rel, atmin + atmax, slack0)
        s2 = np.abs(d2) - fma(rel, atmin, slack0)
        s3 = atmax - slack0
        # v_minimum3_f32: a NaN term leaves the lane unsure
        sure = (s1 > 0) & (s2 > 0) & (s3 > 0)
        ans = (tmax > 0) & (d1 > 0) & (d2 > 0)
    return sure, ans


def slab_cons_v(lo, hi, o, inv, minT0):
    """slab_cons_v on slab_cons_ray's per-axis constants: the axis's entry distance lowered and its
    exit distance raised by e_k (a_k goes with the box minimum, b_k with the maximum)."""
    with np.errstate(all="ignore"):
        p = o * inv
        e = np.copysign(CONS_BIAS * np.abs(p), inv).astype(F)
        a = (-p - e).astype(F)
        b = (-p + e).astype(F)
        t1 = fma(lo, inv, a)
        t2 = fma(hi, inv, b)
        tmin = fmax(fmax(fmin(t1[:, 0], t2[:, 0]), fmin(t1[:, 1], t2[:, 1])), fmin(t1[:, 2], t2[:, 2]))
        tmax = fmin(fmin(fmax(t1[:, 0], t2[:, 0]), fmax(t1[:, 1], t2[:, 1])), fmax(t1[:, 2], t2[:, 2]))
        tiny = np.full_like(tmin, TINY)
        minTc = (minT0 * (F(1.0) + CONS_REL)).astype(F)
        c1 = tmax + tiny
        c2 = (tmax - fma(tmin, np.full_like(tmin, F(1.0) - CONS_REL), -tiny)) + tiny
        c3 = minTc - tmin
        return (c1 > 0) & (c2 > 0) & (c3 > 0)


def pairs(scale, limit_kind, seed):
    """N box / ray pairs: origins at `scale` units, boxes a few units away, rays aimed near the
    box (so hits, misses and grazing rays all occur), for half the pairs one direction component
    scaled down to 1e-6; positive ray limits; reciprocals one ulp either way."""
    rng = np.random.default_rng(seed)
    o = (scale * rng.uniform(-1, 1, (N, 3))).astype(F)
    c = o.astype(np.float64) + rng.uniform(-4, 4, (N, 3))
    h = rng.uniform(0.01, 0.8, (N, 3))
    lo, hi = (c - h).astype(F), (c + h).astype(F)
    tgt = c + rng.uniform(-1.6, 1.6, (N, 3)) * h
    d = tgt - o.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    small = rng.integers(0, 6, N)            # 0..2: that axis shrunk; 3..5: none
    for k in range(3):
        d[:, k] = np.where(small == k, d[:, k] * 1e-6, d[:, k])
    d = d.astype(F)
    d = np.where(d == 0, F(1e-6), d)         # (exact zeros are off the fast path: never sure, not the model's subject)
    with np.errstate(all="ignore"):
        inv = (F(1.0) / d).astype(F)
        shift = rng.integers(-1, 2, (N, 3))
        inv = np.where(shift < 0, np.nextafter(inv, F(-np.inf)), np.where(shift > 0, np.nextafter(inv, F(np.inf)), inv))
        inv = inv.astype(F)
        if limit_kind == "inf":
            minT = np.full(N, np.inf, F)
        else:
            rnd = rng.uniform(1e-3, 12.0, N)
            if limit_kind == "entry":
                t1 = (lo - o) / d
                t2 = (hi - o) / d
                entry = np.max(np.minimum(t1, t2), axis=1).astype(np.float64)
                near = entry * (1.0 + 1e-6 * rng.uniform(-1, 1, N))
                minT = np.where(np.isfinite(near) & (near > 0), near, rnd).astype(F)
            else:
                minT = rnd.astype(F)
    return lo, hi, o, d, inv, minT


LIMITS = ("inf", "entry", "random")


@pytest.mark.parametrize("scale", [1.0, 1e2, 1e4])
def test_fused_slab_predicates(scale):
    """N pairs per limit kind (no limit; within 1e-6 relative of the box entry; random)."""
    sure_all = []
    for limit_kind in LIMITS:
        lo, hi, o, d, inv, minT = pairs(scale, limit_kind, seed=int(scale) * 10 + len(limit_kind))
        exact = box_hit(lo, hi, o, d, minT)
        sure, ans = box_pass(lo, hi, o, d, inv, minT)
        cons = slab_cons_v(lo, hi, o, inv, minT)
        n_wrong = int(np.sum(sure & (ans != exact)))
        n_lost = int(np.sum(exact & ~cons))
        print(f"scale {scale:g} limit {limit_kind}: sure {np.mean(sure):.3f}, exact keeps {np.mean(exact):.3f}, "
              f"conservative keeps {np.mean(cons):.3f}, wrong {n_wrong}, lost {n_lost}")
        assert n_wrong == 0          # 1. sure => the division form's answer
        assert n_lost == 0           # 2. kept by the division form => kept by the conservative test
        sure_all.append(sure)
    frac = float(np.mean(np.concatenate(sure_all)))
    print(f"scale {scale:g}: sure {frac:.3f} of all pairs")
    if scale <= 1e2:
        assert frac >= 0.30          # 3. the first check is not vacuous
