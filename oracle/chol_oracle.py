"""CPU ORACLE (test infrastructure only) for the banded Cholesky solver of meatmodeler_amd/csrc/chol.hip.

    *** This module is the CHECKER.  Only tests/ may import it.  Nothing under meatmodeler_amd/ may.

* `geometry` restates the dispatch of mm_chol_solve_gated (block count, band in blocks, single launch or launch per
  column, the two-ended split and the grid the single launch reserves), so that a test can assert which path ran.
* The matrix families are seeded and banded (A[i][j] == 0 for |i - j| > hb).  `int_well` / `int_mod` have integer
  entries and an integer solution: A, b and x* are exact in f64 and the true solution needs no reference computation.
* `ld_chol` / `ld_solve`: banded Cholesky (doubled long doubles inside, rounded once) and substitutions in long
  double; `factor_residual`, `backward_error`, `kappa_blocks`: the measures the tests bound; `bar_*`: the bounds
  themselves, shared by the GPU tests and by the CPU test that shows LAPACK meets them.
* `model_chol` / `model_solve`: an f64 restatement of the kernel's ALGORITHM (64-blocks, explicit inverse of every
  diagonal block, panel = A_ik L_kk^-T, substitutions by multiplying with the inverses).  A proxy to print ratios
  against, never a bound.
"""
import functools

import numpy as np
import scipy.linalg as sla

from oracle.ba_oracle import LD

NB = 64
FUSED_MAX_BWB = 15
EPS = 2.0 ** -52

# (n, hb): the dispatch edge each shape sits on is in tests/test_chol_reference_cpu.py::GEOMETRY_TABLE
SHAPES = [(2, 2), (64, 64), (66, 66), (128, 5), (130, 0), (256, 64), (258, 64), (320, 65), (322, 63), (446, 128),
          (1024, 768), (1216, 960), (1216, 961)]
SMALL_SHAPES = [s for s in SHAPES if s[0] <= 446]


# --------------------------------------------------------------------------------------------------------- geometry

def geometry(n, hb, sym, nrhs=1, cu_count=None, avoid_fused=False):
    """The dispatch of mm_chol_solve_gated for mm_chol_solve (sym False) / mm_chol_solve_sym (sym True) with the
    default environment.  cu_count: compute units of the device; a grid that does not fit the budget of co-resident
    workgroups takes the launch-per-column path (None: no budget)."""
    nblk = -(-n // NB)
    bwb = min(-(-hb // NB), nblk)
    fused = nblk >= 2 and 1 <= bwb <= FUSED_MAX_BWB and NB * nblk * n < 2 ** 31 and not avoid_fused
    a, m, b = nblk, 0, 0
    if fused and sym and nrhs == 1 and nblk - bwb >= 4:
        m = bwb
        a = (nblk - m + 1) // 2
        b = nblk - m - a
    g_side = (bwb + 1) + bwb * (bwb - 1) // 2
    grid = 2 * g_side + m * (m + 1) // 2 if b > 0 else g_side
    over_budget = bool(fused and cu_count is not None and grid > cu_count)
    if over_budget:
        fused, a, m, b = False, nblk, 0, 0
    return dict(n=n, hb=hb, nblk=nblk, bwb=bwb, fused=fused, a=a, m=m, b=b, pad=nblk * NB - n,
                grid=grid if fused else 0, two_ended=b > 0, over_budget=over_budget)


# --------------------------------------------------------------------------------------------------------- families

def _band_lower(M, w):
    return np.tril(np.triu(M, -w))


def _int_family(n, hb, seed, shift, nrhs):
    rng = np.random.default_rng([seed, n, hb])
    M = _band_lower(rng.integers(-2, 3, size=(n, n)), hb // 2).astype(np.float64)
    A = M @ M.T + shift * np.eye(n)      # sums of at most n products of small integers: exact in f64 in any order
    X = (rng.integers(1, 9, size=(nrhs, n)) * rng.choice([-1, 1], size=(nrhs, n))).astype(np.float64)
    return A, X @ A, X


def int_well(n, hb, seed=0, nrhs=3):
    """(A, B [nrhs, n], X* [nrhs, n]): M integer in -2..2 on the lower band of width hb // 2, A = M M^T + n I, X*
    non-zero integers in -8..8, B = A X*.  Everything is an integer far below 2^53: exact in f64."""
    return _int_family(n, hb, seed, n, nrhs)


def int_mod(n, hb, seed=0, nrhs=3):
    """The same with + 1 I: moderately conditioned."""
    return _int_family(n, hb, seed, 1, nrhs)


def ill(n, hb, seed=0):
    """(A, b): M normal on the lower band of width hb // 2, A = M M^T + 2^-30 max|A| I (cond about 2^30), b normal."""
    rng = np.random.default_rng([seed, n, hb, 1])
    M = _band_lower(rng.normal(size=(n, n)), hb // 2)
    A = M @ M.T
    A = (A + A.T) / 2
    A += 2.0 ** -30 * np.abs(A).max() * np.eye(n)
    return A, rng.normal(size=n)


def graded(A, b, seed=0, shift=0):
    """(D A D, D b, d): D = diag(2^k_i), k_i integer in [-40, 40] + shift, not monotone.  Exact in f64 (powers of two)."""
    n = A.shape[0]
    rng = np.random.default_rng([seed, n, 2])
    d = np.ldexp(1.0, rng.integers(-40, 41, size=n) + shift)
    return A * d[:, None] * d[None, :], b * d, d


def bandwidth(A):
    i, j = np.nonzero(A)
    return int(np.abs(i - j).max()) if i.size else 0


# ------------------------------------------------------------------------------------------- reference and measures

# Doubled long double ("hi + lo", about 126 bits) from error-free transformations: the factor of a matrix with
# cond(A) = 2^31 moves by cond(A) 2^-64 when a single operation rounds to long double, so a reference that is to agree
# with the exact factor to a few units of 2^-63 has to carry more than one long double through the elimination.

_SPLIT = LD(2) ** 32 + LD(1)      # Veltkamp splitter for a 64-bit significand: two halves of 32 bits


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _fast_two_sum(a, b):      # |a| >= |b|
    s = a + b
    return s, b - (s - a)


def _halves(a):
    t = _SPLIT * a
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _halves(a)
    bh, bl = _halves(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_mul(ah, al, bh, bl):
    p, e = _two_prod(ah, bh)
    return _fast_two_sum(p, e + (ah * bl + al * bh))


def _dd_sub(ah, al, bh, bl):
    s, e = _two_sum(ah, -bh)
    return _fast_two_sum(s, e + (al - bl))


def _dd_div(ah, al, bh, bl):
    q1 = ah / bh
    rh, rl = _dd_sub(ah, al, *_dd_mul(q1, 0 * q1, bh, bl))
    q2 = rh / bh
    rh, rl = _dd_sub(rh, rl, *_dd_mul(q2, 0 * q2, bh, bl))
    q3 = rh / bh
    qh, ql = _fast_two_sum(q1, q2)
    return _fast_two_sum(qh, ql + q3)


def _dd_sqrt(ah, al):
    x = 1 / np.sqrt(ah)
    ax = ah * x
    rh, _ = _dd_sub(ah, al, *_two_prod(ax, ax))
    return _fast_two_sum(ax, rh * (x / 2))


def ld_chol(A, hb=None, doubled=True):
    """Lower Cholesky factor of the banded SPD matrix A, returned in long double (column by column, inside the band).
    doubled: the elimination carries doubled long doubles, the result is the factor of A rounded once (to about
    2^-64 entry by entry, whatever cond(A) below 2^60); False: plain long double arithmetic (error cond(A) 2^-64)."""
    A = np.asarray(A).astype(LD)
    n = A.shape[0]
    hb = n if hb is None else hb
    L = np.zeros((n, n), LD)
    Ll = np.zeros((n, n), LD)      # (low parts; stay zero when not doubled)
    for j in range(n):
        lo, hi = max(0, j - hb), min(n, j + hb + 1)
        if not doubled:
            row = L[j, lo:j]
            d = A[j, j] - row @ row
            if not d > 0:
                raise np.linalg.LinAlgError(f"pivot {j + 1} is not positive")
            L[j, j] = np.sqrt(d)
            if hi > j + 1:
                L[j + 1:hi, j] = (A[j + 1:hi, j] - L[j + 1:hi, lo:j] @ row) / L[j, j]
            continue
        sh, sl = A[j:hi, j].copy(), np.zeros(hi - j, LD)      # rows j .. hi - 1 of column j
        for k in range(lo, j):
            sh, sl = _dd_sub(sh, sl, *_dd_mul(L[j:hi, k], Ll[j:hi, k], L[j, k], Ll[j, k]))
        if not sh[0] > 0:
            raise np.linalg.LinAlgError(f"pivot {j + 1} is not positive")
        dh, dl = _dd_sqrt(sh[0], sl[0])
        L[j, j], Ll[j, j] = dh, dl
        if hi > j + 1:
            L[j + 1:hi, j], Ll[j + 1:hi, j] = _dd_div(sh[1:], sl[1:], dh, dl)
    return L


def ld_solve(L, b, hb=None):
    """x of L L^T x = b in long double."""
    L = np.asarray(L).astype(LD)
    n = L.shape[0]
    hb = n if hb is None else hb
    y = np.asarray(b).astype(LD).copy()
    for j in range(n):
        lo = max(0, j - hb)
        y[j] = (y[j] - L[j, lo:j] @ y[lo:j]) / L[j, j]
    for j in range(n - 1, -1, -1):
        hi = min(n, j + hb + 1)
        y[j] = (y[j] - L[j + 1:hi, j] @ y[j + 1:hi]) / L[j, j]
    return y


def factor_residual(A, L):
    """|A - L L^T|_F / (eps |A|_F), evaluated in long double (L: lower triangle; A symmetric).  By 64-row slabs over
    the columns L's own non-zeros reach, the strict lower triangle counted twice."""
    A = np.asarray(A)
    L = np.tril(np.asarray(L)).astype(LD)
    n = A.shape[0]
    w = bandwidth(L)
    total = LD(0)
    for i0 in range(0, n, NB):
        i1 = min(n, i0 + NB)
        lo = max(0, i0 - w)
        R = A[i0:i1, :i1].astype(LD)
        R[:, lo:] -= L[i0:i1, lo:i1] @ L[lo:i1, lo:i1].T
        R = np.tril(R, i0)
        total += 2 * (R ** 2).sum() - (np.diagonal(R, i0) ** 2).sum()
    return float(np.sqrt(total) / (EPS * np.linalg.norm(A.astype(LD))))


def forward_error(x, x_true):
    """max|x - x*| / max|x*|."""
    x, x_true = np.asarray(x).astype(LD), np.asarray(x_true).astype(LD)
    return float(np.abs(x - x_true).max() / np.abs(x_true).max())


def backward_error(A, b, x):
    """eta of the diagonally scaled system (long double): |A^ x^ - b^|inf / (|A^|inf |x^|inf + |b^|inf), A^ = D^-1 A
    D^-1, D = sqrt(diag A) -- the definition of tests/test_ba_reference_gpu.py::_backward_error."""
    A, b, x = (np.asarray(a).astype(LD) for a in (A, b, x))
    d = np.sqrt(np.diag(A))
    Ah = A / d[:, None] / d[None, :]
    bh, xh = b / d, x * d
    r = Ah @ xh - bh
    return float(np.abs(r).max() / (np.abs(Ah).sum(1).max() * np.abs(xh).max() + np.abs(bh).max()))


def scaled(A):
    d = np.sqrt(np.diag(A))
    return A / d[:, None] / d[None, :]


def kappa_blocks(A):
    """max cond of the 64 x 64 diagonal blocks of LAPACK's factor of the diagonally scaled system."""
    Lf = np.linalg.cholesky(scaled(np.asarray(A, np.float64)))
    n = Lf.shape[0]
    return float(max(np.linalg.cond(Lf[i:i + NB, i:i + NB]) for i in range(0, n, NB)))


def _cond_spd(A):
    ev = np.linalg.eigvalsh(A)
    return float(ev[-1] / ev[0])


def lapack_solve(A, b):
    """(L, x) of scipy.linalg.cho_factor / cho_solve; b [n] or [nrhs, n]."""
    c = sla.cho_factor(A, lower=True)
    x = sla.cho_solve(c, np.asarray(b).T).T
    return np.tril(c[0]), x


def lapack_info(A):
    """info of LAPACK's dpotrf on the lower triangle (0: factored; k > 0: the leading minor of order k is not positive
    definite)."""
    return int(sla.lapack.dpotrf(np.asarray(A, np.float64), lower=1)[1])


# ------------------------------------------------------------------------------------------------------------- bars

def bar_forward(fe_lapack):
    """A: fe <= 8 max(fe_LAPACK, 4 eps)."""
    return 8 * max(fe_lapack, 4 * EPS)


def bar_factor_well(rho_lapack):
    """B, well-conditioned: rho <= 8 max(rho_LAPACK, 1)   (rho in units of eps |A|_F)."""
    return 8 * max(rho_lapack, 1.0)


def bar_factor_ill(n, kappa):
    """B, ill-conditioned: rho <= n kappa(L_kk)   (the BA reference suite's formula; rho is already in eps units)."""
    return n * kappa


def bar_backward(n, kappa):
    """C: eta <= n eps kappa(L_kk)."""
    return n * EPS * kappa


# ------------------------------------------------------------------------------------------------------------ model

def model_chol(A, hb=None):
    """(L, [L_kk^-1]) by the kernel's algorithm in f64: right-looking over 64-blocks, the diagonal block factored,
    inverted explicitly by forward substitution without pivoting, panel = A_ik L_kk^-T."""
    A = np.tril(np.asarray(A, np.float64)).copy()
    n = A.shape[0]
    nblk = -(-n // NB)
    bwb = nblk if hb is None else min(-(-hb // NB), nblk)
    inv = []
    for k in range(nblk):
        k0, k1 = k * NB, min(n, (k + 1) * NB)
        Lkk = np.linalg.cholesky(A[k0:k1, k0:k1])
        X = sla.solve_triangular(Lkk, np.eye(k1 - k0), lower=True)
        A[k0:k1, k0:k1] = Lkk
        inv.append(X)
        end = min(n, k1 + bwb * NB)
        if end > k1:
            A[k1:end, k0:k1] = A[k1:end, k0:k1] @ X.T
            P = A[k1:end, k0:k1]
            A[k1:end, k1:end] -= np.tril(P @ P.T)
    return A, inv


def model_solve(L, inv, b, hb=None):
    """x of L L^T x = b by multiplying with the explicit inverses of the diagonal blocks."""
    n = L.shape[0]
    nblk = len(inv)
    bwb = nblk if hb is None else min(-(-hb // NB), nblk)
    x = np.asarray(b, np.float64).copy()
    for k in range(nblk):
        k0, k1 = k * NB, min(n, (k + 1) * NB)
        lo = max(0, k0 - bwb * NB)
        x[k0:k1] = inv[k] @ (x[k0:k1] - L[k0:k1, lo:k0] @ x[lo:k0])
    for k in range(nblk - 1, -1, -1):
        k0, k1 = k * NB, min(n, (k + 1) * NB)
        hi = min(n, k1 + bwb * NB)
        x[k0:k1] = inv[k].T @ (x[k0:k1] - L[k1:hi, k0:k1].T @ x[k1:hi])
    return x


# ---------------------------------------------------------------------------------- cached cases (built once, shared)

def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(family, n, hb):
    """dict of a family's system at (n, hb) with what LAPACK and the model make of it; arrays are read-only.
    A, B [nrhs, n], X (the exact solution, int families only), L_lapack, X_lapack, kappa, cond, rho_lapack (small n),
    eta_lapack, eta_model (first right-hand side), fe_lapack (int families)."""
    if family == "ill":
        A, b = ill(n, hb)
        B, X = b[None, :], None
    else:
        A, B, X = (int_well if family == "int_well" else int_mod)(n, hb)
    L, Xl = lapack_solve(A, B)
    Lm, inv = model_chol(A, hb)
    xm = model_solve(Lm, inv, B[0], hb)
    out = dict(A=A, B=B, X=X, L_lapack=L, X_lapack=Xl, kappa=kappa_blocks(A), cond=_cond_spd(A),
               eta_lapack=backward_error(A, B[0], Xl[0]), eta_model=backward_error(A, B[0], xm), x_model=xm, L_model=Lm)
    if n <= 446:
        out["rho_lapack"] = factor_residual(A, L)
        out["rho_model"] = factor_residual(A, Lm)
    if X is not None:
        out["fe_lapack"] = [forward_error(Xl[c], X[c]) for c in range(len(X))]
        out["fe_model"] = forward_error(xm, X[0])
    _frozen(*out.values())
    return out


def info_cases(n, hb):
    """[(name, A, expected info)]: E's matrices on int_well at (n, hb); the expectation is column + 1 by construction."""
    A = case("int_well", n, hb)["A"]
    out = []
    cols = sorted({c for c in (0, 63, 64, n - 64, n - 1) if 0 <= c < n})
    for c in cols:
        Ab = A.copy()
        Ab[c, c] = -1.0
        out.append((f"col {c}", Ab, c + 1))
    if len(cols) >= 2:      # two bad columns: the smaller one is reported
        lo = cols[1] if len(cols) > 2 else cols[0]
        Ab = A.copy()
        Ab[cols[-1], cols[-1]] = Ab[lo, lo] = -1.0
        out.append((f"cols {lo} and {cols[-1]}", Ab, lo + 1))
    if n > 65 and hb >= 1:
        Ab = A.copy()
        Ab[63:65, :] = 0.0
        Ab[:, 63:65] = 0.0
        Ab[63:65, 63:65] = [[1.0, 2.0], [2.0, 1.0]]
        out.append(("indefinite pair 63|64", Ab, 65))
    return out
