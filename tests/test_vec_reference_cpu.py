"""CPU: the exact reference of the trust-region vector layer (oracle/vec_oracle.py) against fractions.Fraction, its
restatement of the launch geometry, and -- with a small float64 emulation of the kernels' present summation order -- the
bound (depth + 1) eps sum|a_i b_i| that tests/test_vec_reference_gpu.py asserts, on every shape of that file."""
import ast
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from oracle import vec_oracle as vo

HERE = os.path.dirname(os.path.abspath(__file__))


def _gpu_tables():
    """The shape tables at the top of test_vec_reference_gpu.py (that module cannot be imported without a GPU)."""
    with open(os.path.join(HERE, "test_vec_reference_gpu.py")) as fh:
        tree = ast.parse(fh.read())
    want = {"N_SMALL", "N_LARGE", "GRID_CASES"}
    out = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and getattr(node.targets[0], "id", None) in want:
            out[node.targets[0].id] = ast.literal_eval(node.value)
    assert set(out) == want, sorted(out)
    return out


T = _gpu_tables()
ALL_N = tuple(T["N_SMALL"]) + tuple(T["N_LARGE"])


def _shapes():
    """(n, split, cap) of every launch of the GPU file."""
    for n in ALL_N:
        for s in vo.edge_splits(n, full=n in T["N_SMALL"]):
            yield n, s, vo.GRID_CAP
    for cap, ns in T["GRID_CASES"]:
        for n in ns:
            for s in vo.edge_splits(n, full=False)[1:3]:
                yield n, s, cap


def _frac_round(q):
    """Fraction -> the nearest double (ties to even): Python's own correctly rounded integer division."""
    return q.numerator / q.denominator


def _pairs(rng, count):
    """Random and adversarial operand pairs: magnitudes spanning 2^+-200, products with long low halves."""
    a = rng.normal(size=count) * 2.0 ** rng.integers(-200, 201, size=count)
    b = rng.normal(size=count) * 2.0 ** rng.integers(-200, 201, size=count)
    a[::7] = 1.0 + rng.integers(1, 2 ** 26, size=a[::7].size) * 2.0 ** -52       # (1 + k eps)(1 + m eps): low half k m eps^2
    b[::7] = 1.0 + rng.integers(1, 2 ** 26, size=b[::7].size) * 2.0 ** -52
    a[3::11] = np.ldexp(1.0 + 2.0 ** -27, rng.integers(-200, 201, size=a[3::11].size))
    b[3::11] = np.ldexp(1.0 - 2.0 ** -27, rng.integers(-200, 201, size=b[3::11].size))
    return a, b


def test_two_product_is_exact():
    rng = np.random.default_rng(1)
    a, b = _pairs(rng, 4000)
    hi, lo = vo.two_product(a, b)
    assert np.array_equal(hi, a * b)
    for x, y, h, l in zip(a.tolist(), b.tolist(), hi.tolist(), lo.tolist()):
        assert Fraction(h) + Fraction(l) == Fraction(x) * Fraction(y)
    assert np.count_nonzero(lo) > 3000


def test_fma_is_correctly_rounded():
    rng = np.random.default_rng(2)
    a, b = _pairs(rng, 3000)
    c = rng.normal(size=a.size) * np.abs(a * b) * 2.0 ** rng.integers(-60, 61, size=a.size)
    c[::3] = -(a * b)[::3]                                    # cancelling: the result is the product's low half
    c[1::9] = -(a * b)[1::9] * (1.0 + 2.0 ** -40)
    got = vo.fma(a, b, c)
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        assert g == _frac_round(Fraction(x) * Fraction(y) + Fraction(z))
    hi, lo = vo.two_product(a, b)
    assert np.array_equal(got[::3], lo[::3]) and np.count_nonzero(got != a * b + c) > 300   # (differs from mul + add)


def test_exact_dot_is_correctly_rounded():
    rng = np.random.default_rng(3)
    for trial in range(40):
        n = int(rng.integers(1, 200))
        a, b = _pairs(rng, n)
        if trial % 2:      # cancelling sums: the second half undoes the first but for a few elements
            a = np.concatenate([a, a])
            b = np.concatenate([b, -b])
            b[rng.integers(0, 2 * n)] *= 1.0 + 2.0 ** -30
            perm = rng.permutation(2 * n)
            a, b = a[perm], b[perm]
        exact = sum((Fraction(x) * Fraction(y) for x, y in zip(a.tolist(), b.tolist())), Fraction(0))
        assert vo.exact_dot(a, b) == _frac_round(exact)
        hi, lo = vo.two_product(a, b)
        assert vo.exact_sum(np.concatenate([hi, lo])) == _frac_round(exact) and vo.exact_sum(hi[:0]) == 0.0
        assert vo.abs_dot(a, b) == _frac_round(sum((abs(Fraction(x * y)) for x, y in zip(a.tolist(), b.tolist())), Fraction(0)))
        sd = vo.SplitDot(a, b)
        for s in (0, 1, a.size // 2, a.size, a.size + 3):
            ex, ab = sd.columns(s)
            assert ex.tolist() == [vo.exact_dot(a[:s], b[:s]), vo.exact_dot(a[s:], b[s:]), vo.exact_dot(a, b)]
            assert ab.tolist() == [vo.abs_dot(a[:s], b[:s]), vo.abs_dot(a[s:], b[s:]), vo.abs_dot(a, b)]


def _fr(a):
    return [Fraction(v) for v in np.asarray(a, np.float64).tolist()]


def _fsqrt(q):
    """Correctly rounded square root of a positive Fraction (of a double: math.sqrt is correctly rounded)."""
    return Fraction(math.sqrt(float(q)))


@pytest.mark.parametrize("op", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("n,split", [(1, 0), (1, 1), (7, 3), (64, 0), (64, 64), (63, 32)])
def test_fused_reference_vs_fractions(op, n, split):
    """Every op's outputs from Fractions: each operation evaluated exactly and rounded once where IEEE rounds once."""
    rng = np.random.default_rng(10 * n + op)
    r = lambda m=n: rng.normal(size=m) * 2.0 ** rng.integers(-8, 9, size=m)      # noqa: E731
    si = rng.uniform(0.5, 2.0, size=n)
    rd = _frac_round
    if op == 0:
        g = r()
        (gh,), (ghs,) = ([a for _, a in c] for c in vo.fused_reference(0, [g, si]))
        want = [rd(x / s) for x, s in zip(_fr(g), _fr(si))]
        assert gh.tolist() == want and ghs.tolist() == [rd(Fraction(x) / s) for x, s in zip(want, _fr(si))]
    elif op == 1:
        v, dp, gh, gh2 = r(split), r(n - split), r(), np.array([3.7123])
        (gn,), (q1,) = ([a for _, a in c] for c in vo.fused_reference(1, [v, dp, si, gh], [gh2], split=split))
        rt = _fsqrt(Fraction(3.7123))
        assert gn.tolist() == [rd(x * s) for x, s in zip(_fr(np.concatenate([v, dp])), _fr(si))]
        assert q1.tolist() == [rd(x / rt) for x in _fr(gh)]
    elif op == 2:
        gn, q1, sc = r(), r(), np.array([-0.8317])
        cands = dict(vo.fused_reference(2, [gn, q1], [sc])[0])
        s = Fraction(-0.8317)
        assert cands["fma(-sc, q1, gn)"].tolist() == [rd(a - s * b) for a, b in zip(_fr(gn), _fr(q1))]
        assert cands["mul, sub"].tolist() == [rd(a - Fraction(rd(s * b))) for a, b in zip(_fr(gn), _fr(q1))]
    elif op == 3:
        w, q1, wn2 = r(), r(), np.array([0.01934])
        (q2,), (s1,), (s2,) = ([a for _, a in c] for c in vo.fused_reference(3, [w, q1, si, r(), r()], [wn2]))
        rt = _fsqrt(Fraction(0.01934))
        want = [rd(x / rt) for x in _fr(w)]
        assert q2.tolist() == want and s1.tolist() == [rd(x / s) for x, s in zip(_fr(q1), _fr(si))]
        assert s2.tolist() == [rd(Fraction(x) / s) for x, s in zip(want, _fr(si))]
    elif op == 4:
        x, s1, s2, h0, h1 = r(), r(), r(), 0.3127, -1.7093
        cands = dict(vo.fused_reference(4, [x, s1, s2], h0=h0, h1=h1)[0])
        assert len(cands) == 4
        f0, f1 = Fraction(h0), Fraction(h1)
        for fuse0 in (False, True):
            t = [rd(a + f0 * b) if fuse0 else rd(a + Fraction(rd(f0 * b))) for a, b in zip(_fr(x), _fr(s1))]
            name = "fma(h0, s1, x)" if fuse0 else "x + h0*s1"
            assert cands[f"fma(h1, s2, {name})"].tolist() == [rd(Fraction(a) + f1 * b) for a, b in zip(t, _fr(s2))]
            assert cands[f"({name}) + h1*s2"].tolist() == [rd(Fraction(a) + Fraction(rd(f1 * b))) for a, b in zip(t, _fr(s2))]
    else:
        x, s1, s2 = r(), r(), r()
        for p in ([0.4173, -0.2291], [0.4173, 0.0]):
            s2_in = s2 if p[1] else np.full(n, np.nan)          # (never read with p[1] == 0)
            out = vo.fused_reference(5, [x, s1, s2_in], [np.array(p)])[0][0][1]
            t = [rd(a + Fraction(p[0]) * b) for a, b in zip(_fr(x), _fr(s1))]
            if p[1]:
                t = [rd(Fraction(a) + Fraction(p[1]) * b) for a, b in zip(t, _fr(s2))]
            assert out.tolist() == t


def test_partition_tiles_the_vector():
    seen_odd_per = False
    for kind in ("dot", "fused"):
        for cap, ns in [(vo.GRID_CAP, ALL_N)] + [tuple(c) for c in T["GRID_CASES"]]:
            for n in ns:
                p = vo.partition(n, kind, cap)
                grid, per, bounds = p["grid"], p["per"], p["bounds"]
                assert grid == min(max(-(-n // 2048), 1), cap) and len(bounds) == grid
                assert bounds[0][0] == 0 and bounds[-1][1] == n
                assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))          # no gap, no overlap
                assert all(0 <= hi - lo <= per for lo, hi in bounds)
                raw = -(-n // grid)
                if kind == "fused":
                    assert per % 2 == 0 and per in (raw, raw + 1) and all(lo % 2 == 0 or lo == n for lo, _ in bounds)
                    seen_odd_per |= raw % 2 == 1 and grid == cap
                    # the 16-byte pairs the kernel forms are (i, i + 1) with i - lo even and i + 1 < hi: none of them has
                    # its first element below an even split and its second at or above it
                    for s in vo.edge_splits(n, full=n in T["N_SMALL"]):
                        if s % 2 == 0:
                            assert not any(lo <= s - 1 and s < hi and (s - 1 - lo) % 2 == 0 for lo, hi in bounds)
                else:
                    assert per == raw
    assert seen_odd_per                                          # (the cap is where ceil(n / grid) first turns odd)
    assert vo.partition(1, "dot")["depth"] == 1 + 14 + 1 + 14 + 1 and vo.partition(1, "fused")["depth"] == 2 + 14 + 1 + 14 + 1
    assert vo.partition(2048 * 2048 + 3, "fused", 2048)["depth"] == 2 * 3 + 14 + 4 + 14 + 1


def test_grid_cap_reads_the_environment(monkeypatch):
    for val, want in (("1", 1), ("2048", 2048), ("5000", 2048), ("0", 1), ("-3", 1), ("x", 1), ("384", 384)):
        monkeypatch.setenv("MM_VEC_GRID", val)
        assert vo.grid_cap() == want
    monkeypatch.delenv("MM_VEC_GRID")
    assert vo.grid_cap() == 256


# ---- the kernels' present summation order in float64 (numpy rounds every operation once, like the device without
#      contraction; a contracted multiply-add only removes a rounding)

def _tree(v):
    """block_sum_n on [..., 512] thread values -> thread 0's result: 6 shuffle steps per wave, waves in index order."""
    v = v.reshape(v.shape[:-1] + (vo.THREADS // vo.WAVE, vo.WAVE)).copy()
    off = vo.WAVE // 2
    while off:
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    t = np.zeros(v.shape[:-2])
    for w in range(v.shape[-2]):
        t = t + v[..., w, 0]
    return t


def _emulate(terms, kind, cap, pairs):
    """Sum of `terms` (one column: zeros outside its part) the way the kernels add them."""
    n = terms.size
    p = vo.partition(n, kind, cap)
    grid, per = p["grid"], p["per"]
    step = vo.THREADS * (2 if kind == "fused" else 1)
    trips = -(-per // step)
    idx = (per * np.arange(grid))[:, None] + np.arange(trips * step)[None, :]
    ok = (np.arange(trips * step)[None, :] < per) & (idx < n)
    a = np.where(ok, terms[np.minimum(idx, n - 1)], 0.0)
    acc = np.zeros((grid, vo.THREADS))
    if kind == "dot":
        a = a.reshape(grid, trips, vo.THREADS)
        for t in range(trips):
            acc = acc + a[:, t]
    else:
        a = a.reshape(grid, trips, vo.THREADS, 2)
        for t in range(trips):
            if pairs:
                acc = acc + (a[:, t, :, 0] + a[:, t, :, 1])
            else:
                acc = (acc + a[:, t, :, 0]) + a[:, t, :, 1]
    part = _tree(acc)                                            # [grid]
    t2 = -(-grid // vo.THREADS)
    b = np.zeros(t2 * vo.THREADS)
    b[:grid] = part
    acc = np.zeros(vo.THREADS)
    for t in range(t2):
        acc = acc + b[t * vo.THREADS:(t + 1) * vo.THREADS]
    return float(_tree(acc))


def test_summation_order_meets_the_depth_bound():
    """The bound of the GPU file is a property of the reference and the geometry, checked here before any GPU run: the
    emulated sums of all three columns stay within (depth + 1) eps abs_dot on every shape."""
    rng = np.random.default_rng(7)
    worst = 0.0
    data = {}
    for n, split, cap in _shapes():
        if n not in data:
            a = rng.normal(size=n) * 2.0 ** rng.integers(-6, 7, size=n)
            b = rng.normal(size=n)
            data[n] = (a * b, vo.SplitDot(a, b))
        prod, sd = data[n]
        exact, absd = sd.columns(split)
        i = np.arange(n)
        for kind, pairs in (("dot", False), ("fused", split % 2 == 0), ("fused", False)):
            cam = _emulate(np.where(i < split, prod, 0.0), kind, cap, pairs)
            pt = _emulate(np.where(i >= split, prod, 0.0), kind, cap, pairs)
            got = np.array([cam, pt, cam + pt])
            bound = vo.sum_bound(n, kind, absd, cap)
            err = np.abs(got - exact)
            assert np.isfinite(got).all() and (err <= bound).all(), (n, split, cap, kind, pairs, err, bound)
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    assert 0.0 < worst <= 1.0
    print(f"  emulated order: worst err/bound {worst:.3g}")
