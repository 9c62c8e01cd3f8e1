"""CPU: the oracle of the banded Cholesky tests (oracle/chol_oracle.py) -- its matrix families are what they claim,
its long double reference agrees with 50-digit arithmetic, its restatement of the dispatch reproduces the table of
shapes, and LAPACK meets every bound tests/test_chol_reference_gpu.py sets, through the same helper functions."""
import numpy as np
import pytest

from oracle import chol_oracle as co


# (n, hb): nblk, bwb, single launch?, then for mm_chol_solve_sym: (a, m, b), pad, grid -- worked out by hand from
# mm_chol_solve_gated: bwb = min(ceil(hb / 64), nblk); single launch iff nblk >= 2 and 1 <= bwb <= 15; two-ended iff
# nblk - bwb >= 4 with m = bwb, a = (nblk - m + 1) / 2, b = nblk - m - a; G_side = (bwb + 1) + bwb (bwb - 1) / 2
GEOMETRY_TABLE = {
    (2, 2): (1, 1, False, (1, 0, 0), 62, 0),               # diagonal kernel only, per-column path
    (64, 64): (1, 1, False, (1, 0, 0), 0, 0),
    (66, 66): (2, 2, True, (2, 0, 0), 62, 4),              # smallest single launch, pad 62
    (128, 5): (2, 1, True, (2, 0, 0), 0, 2),               # single launch, no pad
    (130, 0): (3, 0, False, (3, 0, 0), 62, 0),             # diagonal matrix, bwb = 0 -> per column
    (256, 64): (4, 1, True, (4, 0, 0), 0, 2),              # nblk - bwb = 3: one-ended even for _sym
    (258, 64): (5, 1, True, (2, 1, 2), 62, 5),             # smallest two-ended, pad 62
    (320, 65): (5, 2, True, (5, 0, 0), 0, 4),              # hb 64 -> 65 makes bwb 2: back to one-ended
    (322, 63): (6, 1, True, (3, 1, 2), 62, 5),             # two-ended, odd split
    (446, 128): (7, 2, True, (3, 2, 2), 2, 11),            # two-ended, pad 2
    (1024, 768): (16, 12, True, (2, 12, 2), 0, 236),       # widest two-ended grid that fits 256 compute units
    (1216, 960): (19, 15, True, (2, 15, 2), 0, 362),       # widest single launch (two-ended: more than 256 workgroups)
    (1216, 961): (19, 16, False, (19, 0, 0), 0, 0),        # one past it: launch per column
}


def test_geometry_reproduces_the_table_of_shapes():
    assert sorted(GEOMETRY_TABLE) == sorted(co.SHAPES)
    for (n, hb), (nblk, bwb, fused, amb, pad, grid) in GEOMETRY_TABLE.items():
        g = co.geometry(n, hb, sym=True)
        assert (g["nblk"], g["bwb"], g["fused"], (g["a"], g["m"], g["b"]), g["pad"], g["grid"]) == \
            (nblk, bwb, fused, amb, pad, grid), (n, hb, g)
        assert g["a"] + g["m"] + g["b"] == nblk and g["two_ended"] == (amb[2] > 0)
        # mm_chol_solve, and mm_chol_solve_sym with several right-hand sides, are one-ended on one side's grid
        g_side = (bwb + 1) + bwb * (bwb - 1) // 2 if fused else 0
        for g1 in (co.geometry(n, hb, sym=False), co.geometry(n, hb, sym=True, nrhs=3)):
            assert (g1["fused"], g1["a"], g1["m"], g1["b"], g1["grid"]) == (fused, nblk, 0, 0, g_side), (n, hb, g1)
        assert not co.geometry(n, hb, sym=True, avoid_fused=True)["fused"]
    # a grid beyond the device's compute units takes the launch-per-column path: the two-ended 1216 / 960 on 256 units
    g = co.geometry(1216, 960, sym=True, cu_count=256)
    assert g["over_budget"] and not g["fused"] and g["grid"] == 0 and (g["a"], g["b"]) == (19, 0)
    g = co.geometry(1216, 960, sym=False, cu_count=256)
    assert g["fused"] and g["grid"] == 121 and not g["over_budget"]
    assert co.geometry(130, 130, sym=False)["grid"] == 7 and co.geometry(130, 130, sym=False)["bwb"] == 3


@pytest.mark.parametrize("n,hb", co.SHAPES)
def test_families_are_banded_exact_and_conditioned_as_stated(n, hb):
    for fam in ("int_well", "int_mod", "ill"):
        if fam == "ill" and n > 446:
            continue
        c = co.case(fam, n, hb)
        A = c["A"]
        assert co.bandwidth(A) <= hb and (A == A.T).all() and np.isfinite(A).all(), (fam, n, hb)
        # what the GPU file's bounds are quoted for (cond, kappa of the 64 x 64 diagonal blocks of LAPACK's factor)
        wide = hb >= 63 and n >= 64
        if fam == "int_well":
            assert 1 <= c["cond"] <= 5 and 1 <= c["kappa"] <= 2.5, (n, hb, c["cond"], c["kappa"])
        elif fam == "int_mod":
            assert c["cond"] <= 4e3 and c["kappa"] <= 20, (n, hb, c["cond"], c["kappa"])
            if wide:
                assert c["cond"] >= 2e2 and c["kappa"] >= 14, (n, hb, c["cond"], c["kappa"])
        else:
            assert c["cond"] <= 4e9, (n, hb, c["cond"])
            if wide:
                assert c["cond"] >= 1e9 and c["kappa"] >= 1e4, (n, hb, c["cond"], c["kappa"])
        if fam != "ill":      # integers: exact arithmetic in int64 at every shape, in Python's own integers at the small ones
            Ai, Xi, Bi = (np.rint(c[k]).astype(np.int64) for k in ("A", "X", "B"))
            assert (Ai == A).all() and (Xi == c["X"]).all() and (Bi == c["B"]).all()
            assert (np.diag(Ai) >= (n if fam == "int_well" else 1)).all()
            assert (np.abs(Xi) >= 1).all() and (np.abs(Xi) <= 8).all()
            assert (Xi @ Ai == Bi).all() and np.abs(Ai).sum(1).max() * 8 < 2 ** 53, (fam, n, hb)
            if n <= 130:
                rows = [[int(v) for v in row] for row in A]
                for X, B in zip(c["X"], c["B"]):
                    xi = [int(v) for v in X]
                    assert [sum(a * x for a, x in zip(row, xi)) for row in rows] == [int(v) for v in B], (fam, n, hb)
    assert (co.case("int_well", n, hb)["A"] - co.case("int_mod", n, hb)["A"] == (n - 1) * np.eye(n)).all()


def test_graded_is_an_exact_power_of_two_scaling():
    A, B, _ = co.int_well(66, 66)
    for shift in (0, 70):
        As, bs, d = co.graded(A, B[0], shift=shift)
        k = np.log2(d)
        assert (k == np.rint(k)).all() and k.min() >= shift - 40 and k.max() <= shift + 40
        assert (np.diff(k) > 0).any() and (np.diff(k) < 0).any()
        assert (As / d[:, None] / d[None, :] == A).all() and (bs / d == B[0]).all()


def _mp_factor_errors(A, hb, doubled=True):
    """ld_chol(A) against mpmath.cholesky at 50 digits: (worst entrywise relative error of L, worst entry of
    |A - L L^T| / (|L| |L|^T) with the products evaluated at 50 digits)."""
    import mpmath
    n = A.shape[0]
    L = co.ld_chol(A, hb, doubled=doubled)
    with mpmath.workdps(50):
        Lm = mpmath.cholesky(mpmath.matrix(A.tolist()))
        Lx = [[_ld_to_mpf(L[i, j]) for j in range(n)] for i in range(n)]
        fwd = max(float(abs(Lx[i][j] - Lm[i, j]) / abs(Lm[i, j])) for i in range(n) for j in range(i + 1) if Lm[i, j] != 0)
        res = 0.0
        for i in range(n):
            for j in range(i + 1):
                s = mpmath.fsum(Lx[i][k] * Lx[j][k] for k in range(j + 1))
                sa = mpmath.fsum(abs(Lx[i][k] * Lx[j][k]) for k in range(j + 1))
                if sa != 0:
                    res = max(res, float(abs(mpmath.mpf(float(A[i, j])) - s) / sa))
    return fwd, res


def test_long_double_reference_against_50_digits():
    """ld_chol against mpmath.cholesky at 50 digits on a 66 x 66 `ill` matrix, entry by entry, to 64 * 2^-63 relative.
    The factor of a matrix with cond(A) = 2.7e9 moves by cond(A) 2^-64 = 1.4e-10 when one operation of the elimination
    rounds to long double (plain long double arithmetic: 3.5e-11 here, LAPACK in f64: 4.5e-7), which is why ld_chol
    carries doubled long doubles and rounds once at the end: measured 5.2e-20, 0.96 * 2^-64."""
    pytest.importorskip("mpmath")
    if np.finfo(co.LD).nmant < 63:
        pytest.skip("long double is no wider than double here")
    A, _ = co.ill(66, 66)
    worst, _ = _mp_factor_errors(A, 66)
    print(f"  ld_chol against mpmath: worst relative error {worst:.3g} (bar {64 * 2.0 ** -63:.3g})")
    assert worst <= 64 * 2.0 ** -63


def test_long_double_reference_residual_against_50_digits():
    """The residual form of the same, for both arithmetics of ld_chol: |A - L L^T| <= 64 * 2^-63 |L| |L|^T entry by entry,
    the products summed at 50 digits (the textbook bound for plain long double is gamma_{n+1} = 67 * 2^-64 at n = 66),
    on the `ill` and the `int_well` matrix; and the substitutions: the long double solution of the integer system is
    the exact one to 2^-58."""
    pytest.importorskip("mpmath")
    if np.finfo(co.LD).nmant < 63:
        pytest.skip("long double is no wider than double here")
    A, b = co.ill(66, 66)
    Aw, Bw, Xw = co.int_well(66, 66)
    for name, M in (("ill", A), ("int_well", Aw)):
        for doubled in (True, False):
            fwd, res = _mp_factor_errors(M, 66, doubled)
            print(f"  {name} doubled={doubled}: residual {res:.3g} of |L||L|^T (bar {64 * 2.0 ** -63:.3g}), factor "
                  f"entrywise {fwd:.3g}")
            assert res <= 64 * 2.0 ** -63
    x = co.ld_solve(co.ld_chol(A, 66), b, 66)
    assert co.backward_error(A, b, x) <= 2.0 ** -60
    assert co.forward_error(co.ld_solve(co.ld_chol(Aw, 66), Bw[0], 66), Xw[0]) <= 2.0 ** -58


def _ld_to_mpf(v):
    """A long double as an mpf, exactly: hi + lo in f64 (call at >= 64 bits of working precision)."""
    import mpmath
    hi = np.float64(v)
    lo = np.float64(v - co.LD(hi))
    assert co.LD(hi) + co.LD(lo) == v
    return mpmath.mpf(float(hi)) + mpmath.mpf(float(lo))


@pytest.mark.parametrize("n,hb", co.SHAPES)
def test_lapack_meets_every_bound_of_the_gpu_suite(n, hb):
    """A, B, C through the helpers the GPU file uses: the bounds are satisfiable by the reference alone."""
    w = co.case("int_well", n, hb)
    Lb = co.ld_chol(w["A"], hb) if n <= 130 else None
    for c in range(3):
        assert w["fe_lapack"][c] <= co.bar_forward(w["fe_lapack"][c])
        if Lb is not None:      # the long double solve has the exact solution to its own rounding
            assert co.forward_error(co.ld_solve(Lb, w["B"][c], hb), w["X"][c]) <= 2.0 ** -58
    assert w["fe_model"] <= co.bar_forward(w["fe_lapack"][0])
    fams = ["int_mod"] + (["ill"] if n <= 446 else [])
    if n <= 446:
        assert w["rho_lapack"] <= co.bar_factor_well(w["rho_lapack"]) and w["rho_lapack"] <= 8
        assert w["rho_model"] <= co.bar_factor_well(w["rho_lapack"])
        i = co.case("ill", n, hb)
        assert i["rho_lapack"] <= co.bar_factor_ill(n, i["kappa"])
    for fam in fams:
        c = co.case(fam, n, hb)
        assert c["eta_lapack"] <= co.bar_backward(n, c["kappa"]), (fam, n, hb, c["eta_lapack"], c["kappa"])
        print(f"  {fam} {n}/{hb}: cond {c['cond']:.3g} kappa_blk {c['kappa']:.3g} eta LAPACK {c['eta_lapack']:.3g} "
              f"model {c['eta_model']:.3g} bound {co.bar_backward(n, c['kappa']):.3g}")


@pytest.mark.parametrize("n,hb", [(66, 66), (322, 63), (446, 128)])
@pytest.mark.parametrize("shift", [0, 70])
def test_lapack_factor_is_covariant_under_power_of_two_scaling(n, hb, shift):
    """D: chol(D A D) == D chol(A) and the solution D^-1 x, bit for bit."""
    c = co.case("int_well", n, hb)
    As, bs, d = co.graded(c["A"], c["B"][0], shift=shift)
    Ls, xs = co.lapack_solve(As, bs)
    assert (Ls == d[:, None] * c["L_lapack"]).all()
    assert (xs == c["X_lapack"][0] / d).all()
    Lm, inv = co.model_chol(As, hb)
    assert (Lm == d[:, None] * c["L_model"]).all()
    assert (co.model_solve(Lm, inv, bs, hb) == c["x_model"] / d).all()


@pytest.mark.parametrize("n,hb", [(64, 64), (130, 130), (322, 63), (256, 64)])
def test_lapack_info_is_the_first_bad_column(n, hb):
    cases = co.info_cases(n, hb)
    assert len(cases) >= 3
    for name, Ab, want in cases:
        assert co.bandwidth(Ab) <= hb and (Ab == Ab.T).all()
        assert co.lapack_info(Ab) == want, (n, hb, name)
        with pytest.raises(np.linalg.LinAlgError):
            co.ld_chol(Ab, hb, doubled=n > 64)      # (both arithmetics at the small shape)
    assert co.lapack_info(co.case("int_well", n, hb)["A"]) == 0
