"""Exact CPU reference of the trust-region vector layer (meatmodeler_amd/csrc/vec.hip): mm_multi_dot and the fused
element-wise passes mm_trf_fused, ops 0-5.  Pure numpy + math, written for this project.

Three things live here:
  * exactness tools -- two_product (Veltkamp / Dekker), exact_dot, abs_dot, fma, and exact_sum / SplitDot for vectors of
    millions of elements -- whose results are the correctly rounded values of the exact quantities
    (tests/test_vec_reference_cpu.py checks them against fractions.Fraction);
  * fused_reference: the element-wise outputs every op defines (include/meatmodeler.h, the comments above FusedTraits);
  * partition: the launch geometry of both kernels restated, with `depth`, the number of floating-point additions a
    term can pass through, from which the tests' bound (depth + 1) eps sum|a_i b_i| follows.

Nothing here models the ORDER of the kernels' sums: the order is free to change, the bound is what is pinned.
"""
import math
import os

import numpy as np

EPS = 2.0 ** -52          # spacing of doubles at 1; the unit roundoff of round-to-nearest is u = EPS / 2

THREADS = 512             # MD_THREADS
SLICE_UNIT = 4 * THREADS  # elements per workgroup below the grid cap
GRID_CAP = 256            # md_grid_cap() without MM_VEC_GRID
GRID_MAX = 2048           # MD_GRID: capacity of the per-workgroup partials
WAVE = 64


# ------------------------------------------------------------------------------------------------ exactness tools

def _veltkamp(a):
    c = 134217729.0 * a           # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def two_product(a, b):
    """(hi, lo) with hi = fl(a * b) and hi + lo == a * b exactly (Veltkamp splitting, Dekker's product); element-wise,
    float64.  Needs |a|, |b| < 2^996 and a product whose low half does not underflow (|a b| > 2^-968)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    hi = a * b
    ah, al = _veltkamp(a)
    bh, bl = _veltkamp(b)
    lo = al * bl - (((hi - ah * bh) - al * bh) - ah * bl)
    return hi, lo


def exact_dot(a, b):
    """The correctly rounded value of the exact inner product sum a_i b_i."""
    hi, lo = two_product(np.ravel(a), np.ravel(b))
    return math.fsum(hi.tolist() + lo.tolist())


def abs_dot(a, b):
    """sum |a_i b_i| (of the rounded products; correctly rounded sum)."""
    return math.fsum(np.abs(np.ravel(np.asarray(a, np.float64)) * np.ravel(np.asarray(b, np.float64))).tolist())


def fma(a, b, c):
    """Correctly rounded a * b + c per element -- what the hardware's fused multiply-add returns, bit for bit."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    hi, lo = two_product(a, b)
    out = [math.fsum(t) for t in zip(c.ravel().tolist(), hi.ravel().tolist(), lo.ravel().tolist())]
    return np.array(out, dtype=np.float64).reshape(a.shape)


def exact_sum(x):
    """The correctly rounded sum of the doubles x -- math.fsum's value -- for long vectors: mantissas are added as integers
    per exponent (two 27-bit halves, so that every partial sum stays below 2^53 and numpy's float accumulation is exact),
    and math.fsum adds the few hundred exactly representable bin totals."""
    x = np.ravel(np.asarray(x, dtype=np.float64))
    if x.size == 0:
        return 0.0
    assert x.size < 2 ** 25 and np.isfinite(x).all()
    m, e = np.frexp(x)                                  # x = m 2^e with 0.5 <= |m| < 1 (0 for x = 0)
    mi = np.ldexp(m, 53).astype(np.int64)               # x = mi 2^(e - 53), |mi| < 2^53
    top, low = mi >> 27, mi & ((1 << 27) - 1)           # mi = top 2^27 + low, 0 <= low < 2^27, |top| <= 2^26
    e0 = int(e.min())
    idx = (e - e0).astype(np.int64)
    st = np.bincount(idx, weights=top.astype(np.float64))
    sl = np.bincount(idx, weights=low.astype(np.float64))
    ex = np.arange(st.size) + (e0 - 53)
    return math.fsum(np.ldexp(st, ex + 27).tolist() + np.ldexp(sl, ex).tolist())


class SplitDot:
    """exact_dot / abs_dot of one pair of vectors in the kernels' three columns (i < split, i >= split, all) for several
    values of `split`: the exact products are formed once."""

    def __init__(self, a, b):
        a = np.ravel(np.asarray(a, np.float64))
        b = np.ravel(np.asarray(b, np.float64))
        hi, lo = two_product(a, b)
        self.n = a.size
        self._hi, self._lo, self._ab = hi, lo, np.abs(hi)
        self._total = None

    def _part(self, i0, i1):
        return exact_sum(np.concatenate([self._hi[i0:i1], self._lo[i0:i1]])), exact_sum(self._ab[i0:i1])

    def columns(self, split):
        """-> (exact [3], abs [3])."""
        s = min(max(int(split), 0), self.n)
        if self._total is None:
            self._total = self._part(0, self.n)
        cam = self._part(0, s) if 0 < s < self.n else (self._total if s else (0.0, 0.0))
        pt = self._part(s, self.n) if 0 < s < self.n else ((0.0, 0.0) if s else self._total)
        return np.array([cam[0], pt[0], self._total[0]]), np.array([cam[1], pt[1], self._total[1]])


# ------------------------------------------------------------------------------------------- element-wise reference

def fused_reference(op, ins, scalars=(), h0=0.0, h1=0.0, split=0):
    """Element-wise outputs of mm_trf_fused's op: a list with one entry per output vector; every entry is a list of
    (label, array) candidates.  An element of the kernel's output is right if it equals ANY candidate bit for bit.

    Ops 0, 1, 3 are made of IEEE operations with one correct result (/, *, sqrt): one candidate.  Op 5 is written as an
    explicit chain fma(h1, s2, fma(h0, s1, x)), without its second link when h1 == 0 (s2 is then never read): one
    candidate.  Ops 2 and 4 are plain expressions, whose contraction into fused multiply-adds is the compiler's choice:
    every contraction of the left-to-right expression is a candidate."""
    ins = [np.asarray(t, np.float64) for t in ins]
    sc = [np.asarray(t, np.float64).ravel() for t in scalars]
    if op == 0:                                   # gh = g / si, ghs = gh / si
        g, si = ins
        gh = g / si
        return [[("ieee", gh)], [("ieee", gh / si)]]
    if op == 1:                                   # gn = [v ; dp] * si, q1 = gh / sqrt(gh2)
        v, dp, si, gh = ins
        n = si.size
        q = np.concatenate([v[:split], dp[:n - split]])
        return [[("ieee", q * si)], [("ieee", gh / np.sqrt(sc[0][0]))]]
    if op == 2:                                   # w = gn - sc q1
        gn, q1 = ins
        s = sc[0][0]
        return [[("mul, sub", gn - s * q1), ("fma(-sc, q1, gn)", fma(-s, q1, gn))]]
    if op == 3:                                   # q2 = w / sqrt(wn2), s1 = q1 / si, s2 = q2 / si
        w, q1, si = ins[:3]
        q2 = w / np.sqrt(sc[0][0])
        return [[("ieee", q2)], [("ieee", q1 / si)], [("ieee", q2 / si)]]
    if op == 4:                                   # (x + h0 s1) + h1 s2
        x, s1, s2 = ins
        inner = [("x + h0*s1", x + h0 * s1), ("fma(h0, s1, x)", fma(h0, s1, x))]
        cands = []
        for name, t in inner:
            cands.append((f"({name}) + h1*s2", t + h1 * s2))
            cands.append((f"fma(h1, s2, {name})", fma(h1, s2, t)))
        return [cands]
    if op == 5:
        x, s1 = ins[:2]
        p0, p1 = float(sc[0][0]), float(sc[0][1])
        out = fma(p0, s1, x)
        if p1 != 0.0:
            out = fma(p1, ins[2], out)
        return [[("fma chain", out)]]
    raise ValueError(f"op {op}")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def match_candidates(got, cands):
    """-> (mask of elements that equal some candidate bit for bit, {label: number of elements it matches})."""
    gb = bits(got)
    ok = np.zeros(gb.shape, bool)
    counts = {}
    for label, arr in cands:
        m = gb == bits(arr)
        ok |= m
        counts[label] = int(m.sum())
    return ok, counts


# ------------------------------------------------------------------------------------------------- launch geometry

def grid_cap():
    """md_grid_cap(): MM_VEC_GRID (read once per process by the library), clamped to 1 .. 2048; 256 without it."""
    e = os.environ.get("MM_VEC_GRID")
    if e is None:
        return GRID_CAP
    try:
        v = int(e.strip())
    except ValueError:
        v = 0
    return min(max(v, 1), GRID_MAX)


def partition(n, kind, cap=None):
    """Launch geometry of multi_dot_kernel (kind "dot") or fused_vec_kernel (kind "fused") on a vector of n >= 1
    elements: dict(grid, per, bounds, depth).

    grid = ceil(n / 2048) workgroups of 512 threads, at least 1 and at most `cap` (grid_cap() when None).  Workgroup b
    owns [per b, min(n, per b + per)) with per = ceil(n / grid), rounded up to even for the fused passes (so that a
    16-byte pair never straddles two slices, or an even `split`); `bounds` lists the slices, empty ones as (n, n).

    depth: the largest number of floating-point additions a term of a sum can pass through on its way to a result
    column.  Counted from the code (vec.hip and ba_eval.h; line numbers as of this writing), additions to a zero
    accumulator included:

      multi_dot_kernel
        per-thread strided loop, vec.hip:45-53 (stride 512 over the slice): ceil(per / 512) trips,
            one addition per trip                                                          ceil(per / 512)
      fused_vec_body
        per-thread loop, vec.hip:324-336 (two neighbouring elements per trip, stride 1024): t = ceil(per / 1024) trips;
            16-byte path: the pair is summed first (fused_elem2, "p[q] = ..; p[q] += ..", vec.hip:253-287) and then
            added to the accumulator (the `add` lambda, vec.hip:315-323): t + 1 for a term of the first trip;
            element-by-element path: two additions per trip: 2 t.                          max(t + 1, 2 t)
      both, after the loop
        block_sum_n (ba_eval.h:239-257): wave_sum_n's 6 shuffle steps (ba_eval.h:225-234), then thread 0 adds the
            8 waves' sums in index order starting from 0                                   6 + 8 = 14
        the last workgroup's strided loop over the per-workgroup partials (vec.hip:68-72 / 381-387):
            one addition per trip                                                          ceil(grid / 512)
        its tree, the same block_sum_n (vec.hip:73 / 395)                                  14
        total = camera + point (vec.hip:79 / 407)                                          1

    The camera and point columns do without the last addition; the bound uses one depth for all three columns.
    A term therefore carries at most depth + 1 roundings (its product is one more; a compiler that contracts product and
    addition only removes roundings), and  |sum - exact| <= ((1 + u)^(depth + 1) - 1) sum|a_i b_i|  with u = EPS / 2,
    which (depth + 1) EPS sum|a_i b_i| bounds with a factor 2 to spare for the higher-order terms."""
    if kind not in ("dot", "fused"):
        raise ValueError(kind)
    n = int(n)
    if n < 1:
        raise ValueError("n >= 1 (an empty vector launches nothing)")
    cap = grid_cap() if cap is None else int(cap)
    grid = min(max(-(-n // SLICE_UNIT), 1), cap)
    per = -(-n // grid)
    if kind == "fused":
        per = (per + 1) & ~1
        t = -(-per // (2 * THREADS))
        chain = max(t + 1, 2 * t)
    else:
        chain = -(-per // THREADS)
    tree = 6 + THREADS // WAVE
    depth = chain + tree + -(-grid // THREADS) + tree + 1
    bounds = [(min(n, per * b), min(n, per * b + per)) for b in range(grid)]
    return dict(grid=grid, per=per, bounds=bounds, depth=depth)


def sum_bound(n, kind, absd, cap=None):
    """(depth + 1) EPS absd: the bound on |kernel sum - exact sum| for a column whose terms' magnitudes add up to absd."""
    return (partition(n, kind, cap)["depth"] + 1) * EPS * np.asarray(absd, dtype=np.float64)


def edge_splits(n, full=True):
    """Values of `split` at which the partition of an n-vector can go wrong: both ends, the first slice boundary of either
    kernel and its neighbours, and an odd and an even value inside the vector (full = False: only the ends and the two
    inner values).  Clipped to [0, n], sorted, without duplicates."""
    odd_mid, even_mid = (5 * n // 8) | 1, ((3 * n // 8) + 1) & ~1
    s = {0, n, odd_mid, even_mid}
    if full:
        s |= {1, 2, n - 1}
        for kind in ("dot", "fused"):
            per = partition(n, kind, GRID_CAP)["per"]
            s |= {per - 1, per, per + 1}
    return sorted({min(max(v, 0), n) for v in s})
