"""GPU: the banded Cholesky solver (csrc/chol.hip: mm_chol_solve, mm_chol_solve_sym) at its block, band and two-ended
boundaries, against exact solutions, LAPACK-relative bars and the long double measures of oracle/chol_oracle.py.

Every shape sits on a dispatch edge (tests/test_chol_reference_cpu.py::GEOMETRY_TABLE) and every solve asserts the path
it took: single launch or launch per column (CTL_CHOL_LAST_PATH) and one- or two-ended (CTL_CHOL_RESERVED, the grid the
single launch reserved, read before the context synchronises).  With MM_CHOL_FUSED=0 or MM_CHOL_TWISTED=0 in the
environment the path assertions are skipped and everything else holds as it stands.

A  exact-truth solutions (integer systems): fe <= 8 max(fe_LAPACK, 4 eps)
B  the factor: rho = |A - L L^T|_F / (eps |A|_F) <= 8 max(rho_LAPACK, 1) (well conditioned), <= n kappa(L_kk) (cond 2e9);
   the strict upper triangle is neither read nor written
C  backward error of the scaled system <= n eps kappa(L_kk)   (the bound of tests/test_ba_reference_gpu.py)
D  power-of-two diagonal scaling commutes with the solver bit for bit
E  info: the first bad column exactly (one-ended), 1..n (two-ended), NaN input, recovery on the same buffers
F  one workspace across shapes and paths: bit-identical to a fresh one (zeros, 0xFF)
G  the argument contract

Measured ratios and the kernel mutations these tests were tried against: DESIGN.md section 6a.

Run on the MI355X box:  python -m pytest tests/test_chol_reference_gpu.py -q -s
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from meatmodeler_amd import ops  # noqa: E402
from meatmodeler_amd._lib import default_context, lib, ptr  # noqa: E402
from oracle import chol_oracle as co  # noqa: E402

DEV = torch.device("cuda", 0)
MM_ERR_ARG, MM_ERR_WORKSPACE = -1, -3


def _env_int(name, default):
    v = os.environ.get(name)
    return default if v is None else int(v)


# the environment's switches move the dispatch away from what geometry() restates: no path assertions then
CHECK_PATH = _env_int("MM_CHOL_FUSED", 2) > 0 and _env_int("MM_CHOL_TWISTED", 1) != 0

HOWS = ("chol", "sym both", "sym lower")


def dev(a):
    return torch.as_tensor(np.array(a, order="C")).to(DEV)      # (a copy: the oracle's cases are read-only)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def nan_upper(A):
    """The lower triangle of A, NaN in the strict upper one."""
    out = np.tril(A)
    out[np.triu_indices(A.shape[0], 1)] = np.nan
    return out


def workspace(n, fill=None):
    wsb = lib.mm_chol_workspace_bytes(n)
    if fill is None:
        return torch.empty(wsb, dtype=torch.uint8, device=DEV)
    return torch.full((wsb,), fill, dtype=torch.uint8, device=DEV)


def solve(how, A, b, hb, ws=None, info=None, avoid=False, check_path=True):
    """One solve through ops.chol_solve / ops.chol_solve_sym (ws is None) or through ctypes on the given workspace and
    info buffer; asserts the path geometry() predicts.  b [n], [nrhs, n] or None (factor only, ctypes).
    -> (info, x, A as it came back)."""
    ctx = default_context()
    n = A.shape[0]
    hb = min(hb, n)
    sym = how != "chol"
    nrhs = 0 if b is None else (1 if np.ndim(b) == 1 else len(b))
    Ad = dev(nan_upper(A) if how == "sym lower" else A)
    bd = None if b is None else dev(b)
    ctx.sync()      # gives back what an earlier solve reserved
    prev = ctx.control(ctx.CTL_CHOL_AVOID_FUSED, 1 if avoid else 0)
    try:
        if ws is None and info is None and b is not None:
            info = ops.chol_solve_sym(Ad, bd, half_bandwidth=hb, both_triangles=how == "sym both") if sym \
                else ops.chol_solve(Ad, bd, half_bandwidth=hb)
        else:
            ws = workspace(n) if ws is None else ws
            info = torch.full((1,), 12345, dtype=torch.int32, device=DEV) if info is None else info
            if sym:
                rc = lib.mm_chol_solve_sym(ctx.h, ptr(Ad), n, ptr(bd), hb, int(how == "sym both"), ptr(info), ptr(ws),
                                           ws.numel())
            else:
                rc = lib.mm_chol_solve(ctx.h, ptr(Ad), n, ptr(bd), nrhs, hb, ptr(info), ptr(ws), ws.numel())
            ctx.check(rc, "mm_chol_solve*")
        path, reserved = int(ctx.control(ctx.CTL_CHOL_LAST_PATH)), int(ctx.control(ctx.CTL_CHOL_RESERVED))
    finally:
        ctx.control(ctx.CTL_CHOL_AVOID_FUSED, prev)
    ctx.sync()
    if CHECK_PATH and check_path:
        g = co.geometry(n, hb, sym, nrhs=nrhs, cu_count=int(ctx.control(ctx.CTL_CU_COUNT)), avoid_fused=avoid)
        assert (path, reserved) == (int(g["fused"]), g["grid"]), (how, n, hb, path, reserved, g)
    return int(info), (None if bd is None else host(bd)), host(Ad)


def describe(n, hb, how, nrhs=1):
    g = co.geometry(n, hb, how != "chol", nrhs=nrhs, cu_count=int(default_context().control(default_context().CTL_CU_COUNT)))
    if not g["fused"]:
        return "per column" + (" (grid over the budget)" if g["over_budget"] else "")
    return f"single launch, {'two-ended a=%d m=%d b=%d' % (g['a'], g['m'], g['b']) if g['two_ended'] else 'one-ended'}"


# ------------------------------------------------------------------------------------------------------------------ A

@pytest.mark.parametrize("n,hb", co.SHAPES)
def test_a_exact_truth_solutions(n, hb):
    c = co.case("int_well", n, hb)
    A, B, X = c["A"], c["B"], c["X"]
    print(f"\nA int_well {n}/{hb}: cond {c['cond']:.3g}")
    for how, nrhs in (("chol", 1), ("chol", 3), ("sym both", 1), ("sym lower", 1)):
        b = B[0] if nrhs == 1 else B
        info, x, _ = solve(how, A, b, hb)
        assert info == 0, (how, nrhs, info)
        x = np.atleast_2d(x)
        assert np.isfinite(x).all(), (how, nrhs)
        for r in range(nrhs):
            fe, fl = co.forward_error(x[r], X[r]), c["fe_lapack"][r]
            print(f"  {how:<9} nrhs {nrhs} rhs {r} [{describe(n, hb, how, nrhs)}]: fe {fe:.3g}  fe/LAPACK "
                  f"{fe / fl if fl else float('inf'):.3g}  fe/bar {fe / co.bar_forward(fl):.3g}")
            assert fe <= co.bar_forward(fl), (how, nrhs, r, fe, fl)
        if nrhs == 3:      # each right-hand side bit for bit as when it is solved alone
            for r in range(3):
                info1, x1, _ = solve("chol", A, B[r], hb)
                assert info1 == 0 and (bits(x1) == bits(x[r])).all(), (r, np.abs(x1 - x[r]).max())


# ------------------------------------------------------------------------------------------------------------------ B

@pytest.mark.parametrize("family", ["int_well", "ill"])
@pytest.mark.parametrize("n,hb", co.SMALL_SHAPES)
def test_b_factor(n, hb, family):
    c = co.case(family, n, hb)
    A, b = c["A"], c["B"][0]
    info, x, Lg = solve("chol", nan_upper(A), b, hb)
    assert info == 0
    iu = np.triu_indices(n, 1)
    assert (bits(Lg[iu]) == bits(np.full(iu[0].size, np.nan))).all(), "the strict upper triangle was written"
    L = np.tril(Lg)
    assert np.isfinite(L).all() and np.isfinite(x).all()
    info2, x2, Lg2 = solve("chol", A, b, hb)
    assert info2 == 0 and (bits(np.tril(Lg2)) == bits(L)).all() and (bits(x2) == bits(x)).all(), \
        "the upper triangle was read"
    assert (bits(Lg2[iu]) == bits(A[iu])).all()
    rho = co.factor_residual(A, L)
    bar = co.bar_factor_well(c["rho_lapack"]) if family == "int_well" else co.bar_factor_ill(n, c["kappa"])
    print(f"\nB {family} {n}/{hb} [{describe(n, hb, 'chol')}]: rho {rho:.3g}  rho/LAPACK {rho / c['rho_lapack']:.3g}  "
          f"rho/model {rho / c['rho_model']:.3g}  rho/bar {rho / bar:.3g}  (cond {c['cond']:.3g} kappa_blk {c['kappa']:.3g})")
    assert rho <= bar, (rho, bar, c["rho_lapack"])


@pytest.mark.parametrize("hb", [0, 5])
def test_b_pivots_of_a_diagonal_matrix(hb):
    """A diagonal matrix (declared band 0: launch per column; 5: single launch): L_ii = A_ii * r with r the refined
    reciprocal square root.  The refinement leaves r within 2^-75 of 1 / sqrt(A_ii) before its final rounding, so L_ii
    carries two roundings: |L_ii - sqrt(A_ii)| <= 2^-52 (1 + 2^-20) sqrt(A_ii) against the long double square root
    (2^-20: slack for the refinement's own arithmetic, generous by 2^30).  Off-diagonal entries stay exact zeros and
    x_i = b_i r r to four roundings (two multiplications by the inverse of L_ii, which is r, rounded once itself)."""
    n = 130
    rng = np.random.default_rng([7, hb])
    dg = rng.uniform(1.0, 4.0, n) * 4.0 ** rng.integers(-20, 21, n)      # every significand, both exponent parities
    dg[:4] = [1.0, 2.0, 3.0, 4.0 - 2.0 ** -50]
    A, b = np.diag(dg), rng.normal(size=n)
    info, x, Lg = solve("chol", A, b, hb)
    assert info == 0
    L = np.tril(Lg)
    assert (L[~np.eye(n, dtype=bool)] == 0).all()
    s = np.sqrt(dg.astype(co.LD))
    err = np.abs(np.diag(L).astype(co.LD) - s) / s
    bar = 2.0 ** -52 * (1 + 2.0 ** -20)
    xerr = np.abs(x.astype(co.LD) - b.astype(co.LD) / dg.astype(co.LD)) / np.abs(b / dg)
    print(f"\nB diagonal {n}/{hb} [{describe(n, hb, 'chol')}]: worst pivot error {float(err.max()) / 2.0 ** -53:.3g} * 2^-53 "
          f"(bar {bar / 2.0 ** -53:.3g}), mean {float(err.mean()) / 2.0 ** -53:.3g};  worst x error "
          f"{float(xerr.max()) / 2.0 ** -53:.3g} * 2^-53 (bar 4)")
    assert float(err.max()) <= bar
    assert float(xerr.max()) <= 4 * 2.0 ** -53 * (1 + 2.0 ** -20)


# ------------------------------------------------------------------------------------------------------------------ C

@pytest.mark.parametrize("n,hb,family", [(n, hb, f) for f in ("ill", "int_mod") for n, hb in co.SMALL_SHAPES] +
                         [(1024, 768, "int_mod"), (1216, 960, "int_mod"), (1216, 961, "int_mod")])
def test_c_backward_error(n, hb, family):
    c = co.case(family, n, hb)
    A, b = c["A"], c["B"][0]
    bar = co.bar_backward(n, c["kappa"])
    print(f"\nC {family} {n}/{hb}: cond {c['cond']:.3g} kappa_blk {c['kappa']:.3g} bar {bar:.3g} "
          f"eta LAPACK {c['eta_lapack']:.3g} model {c['eta_model']:.3g}")
    for how in HOWS:
        info, x, _ = solve(how, A, b, hb)
        assert info == 0, (how, info)
        assert np.isfinite(x).all(), how
        eta = co.backward_error(A, b, x)
        print(f"  {how:<9} [{describe(n, hb, how)}]: eta {eta:.3g}  eta/bar {eta / bar:.3g}  eta/LAPACK "
              f"{eta / c['eta_lapack']:.3g}  eta/model {eta / c['eta_model']:.3g}")
        assert eta <= bar, (how, eta, bar)


# ------------------------------------------------------------------------------------------------------------------ D

@pytest.mark.parametrize("shift", [0, 70])
@pytest.mark.parametrize("n,hb", [(66, 66), (322, 63), (446, 128)])
def test_d_power_of_two_scaling(n, hb, shift):
    """D A D x' = D b with D = diag(2^k_i): every operation of the algorithm commutes with the scaling (pivots scale by
    4^k_i, which the reciprocal square root and its refinement follow exactly), so L' = D L and x' = D^-1 x bit for
    bit.  shift 70 lifts the diagonal of L to 2^30 .. 2^110: far from overflow, beyond any absolute threshold."""
    c = co.case("int_well", n, hb)
    A, b = c["A"], c["B"][0]
    As, bs, d = co.graded(A, b, shift=shift)
    info, x, L = solve("chol", A, b, hb)
    info_s, xs, Ls = solve("chol", As, bs, hb)
    assert info == 0 and info_s == 0, (info, info_s)
    dL = np.abs(bits(np.tril(Ls)) - bits(d[:, None] * np.tril(L))).max()
    dx = np.abs(bits(xs) - bits(x / d)).max()
    print(f"\nD {n}/{hb} shift {shift}: chol factor differs by {dL} ulp, solution by {dx} ulp")
    assert dL == 0 and dx == 0, (dL, dx)
    for how in ("sym both", "sym lower"):
        info, x, _ = solve(how, A, b, hb)
        info_s, xs, _ = solve(how, As, bs, hb)
        assert info == 0 and info_s == 0, (how, info, info_s)
        dx = np.abs(bits(xs) - bits(x / d)).max()
        print(f"  {how} [{describe(n, hb, how)}]: solution differs by {dx} ulp")
        assert dx == 0, (how, dx)


# ------------------------------------------------------------------------------------------------------------------ E

def _recover(how, c, hb, ws, info_t, avoid):
    """A good solve on the buffers a failing one has just used: info 0 and bar A."""
    info, x, _ = solve(how, c["A"], c["B"][0], hb, ws=ws, info=info_t, avoid=avoid)
    assert info == 0, (how, info)
    fe = co.forward_error(x, c["X"][0])
    assert fe <= co.bar_forward(c["fe_lapack"][0]), (how, fe)


@pytest.mark.parametrize("how,n,hb,avoid", [("chol", 64, 64, False), ("chol", 130, 130, True), ("chol", 130, 130, False),
                                            ("chol", 322, 63, False), ("sym both", 256, 64, False),
                                            ("sym lower", 256, 64, False)])
def test_e_info_is_the_first_bad_column(how, n, hb, avoid):
    """One-ended eliminations report what LAPACK's dpotrf reports: the order of the first leading minor that is not
    positive definite."""
    c = co.case("int_well", n, hb)
    ws = workspace(n)
    info_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    b = np.ones(n)
    print(f"\nE {how} {n}/{hb} avoid_fused={avoid} [{'per column' if avoid else describe(n, hb, how)}]")
    for name, Ab, want in co.info_cases(n, hb):
        assert co.lapack_info(Ab) == want, (name, want)
        info, _, _ = solve(how, Ab, b, hb, ws=ws, info=info_t, avoid=avoid)
        print(f"  {name}: info {info} (dpotrf {want})")
        assert info == want, (name, info, want)
        _recover(how, c, hb, ws, info_t, avoid)


@pytest.mark.parametrize("n,hb", [(258, 64), (322, 63)])
def test_e_info_two_ended(n, hb):
    """The two-ended elimination runs in another order than LAPACK's: 1 <= info <= n is all the header promises in
    general.  What follows from the order itself is asserted as well.  Side 0 eliminates columns 0 .. 64 a - 1 exactly
    as LAPACK does and sees nothing of side 1; the middle block is eliminated last, in natural order, from the Schur
    complement of both ends: a bad column there is reported exactly.  On the reversed side a failure spreads towards
    SMALLER columns, down to the middle block at most: info lies between the first column of the middle block and the
    bad one."""
    c = co.case("int_well", n, hb)
    g = co.geometry(n, hb, True)
    assert g["two_ended"]
    ws = workspace(n)
    info_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    cols = {"side 0": 10, "middle": g["a"] * 64 + 10, "side 1": n - 10}
    assert cols["middle"] < (g["a"] + g["m"]) * 64 <= cols["side 1"]
    print(f"\nE two-ended {n}/{hb} a={g['a']} m={g['m']} b={g['b']}")
    for where, col in cols.items():
        Ab = c["A"].copy()
        Ab[col, col] = -1.0
        assert co.lapack_info(Ab) == col + 1
        for how in ("sym both", "sym lower"):
            info, _, _ = solve(how, Ab, np.ones(n), hb, ws=ws, info=info_t)
            print(f"  {where} column {col} {how}: info {info} (dpotrf {col + 1})")
            assert 1 <= info <= n, (where, how, info)
            if CHECK_PATH:
                lo = g["a"] * 64 + 1 if where == "side 1" else col + 1
                assert lo <= info <= col + 1, (where, how, info, lo, col + 1)
            else:      # one-ended (MM_CHOL_TWISTED=0) or per column (MM_CHOL_FUSED=0): LAPACK's value
                assert info == col + 1, (where, how, info)
            _recover(how, c, hb, ws, info_t, False)


@pytest.mark.parametrize("how,n,hb,avoid", [("sym both", 322, 63, False), ("chol", 130, 130, True)])
def test_e_nan_input(how, n, hb, avoid):
    c = co.case("int_well", n, hb)
    Ab = c["A"].copy()
    Ab[70, 40] = Ab[40, 70] = np.nan      # a sub-diagonal entry inside the band, in block (1, 0)
    assert abs(70 - 40) <= hb
    ws = workspace(n)
    info_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    info, _, _ = solve(how, Ab, np.ones(n), hb, ws=ws, info=info_t, avoid=avoid)
    print(f"\nE NaN at (70, 40), {how} {n}/{hb} avoid_fused={avoid}: info {info}")
    assert info > 0, info
    _recover(how, c, hb, ws, info_t, avoid)


# ------------------------------------------------------------------------------------------------------------------ F

def test_f_one_workspace_across_shapes_and_paths():
    """Stale flags, sentinels and inverses of an earlier solve -- of another shape, path and layout -- change nothing."""
    shared = workspace(1216, fill=0)
    info_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    print()
    for step, (how, n, hb) in enumerate([("sym both", 1216, 960), ("sym both", 258, 64), ("chol", 130, 130),
                                         ("chol", 1216, 961), ("chol", 66, 66), ("sym both", 258, 64)]):
        A, B, X = co.int_well(n, hb, nrhs=1)
        runs = [solve(how, A, B[0], hb, ws=shared, info=info_t)]
        for fill in (0, 0xFF):
            runs.append(solve(how, A, B[0], hb, ws=workspace(n, fill=fill)))
        print(f"  F step {step} {how} {n}/{hb} [{describe(n, hb, how)}]: fe {co.forward_error(runs[0][1], X[0]):.3g}")
        for info, x, Ao in runs:
            assert info == 0
            assert (bits(x) == bits(runs[0][1])).all(), (step, how, n, hb, np.abs(x - runs[0][1]).max())
            if how == "chol":
                assert (bits(np.tril(Ao)) == bits(np.tril(runs[0][2]))).all(), (step, n, hb)
        fe_lapack = co.forward_error(co.lapack_solve(A, B[0])[1], X[0])
        assert co.forward_error(runs[0][1], X[0]) <= co.bar_forward(fe_lapack)


# ------------------------------------------------------------------------------------------------------------------ G

def test_g_argument_contract():
    """The refusals come before the first launch (mm_chol_solve_gated checks its arguments first): the context's launch
    log stays empty, A, b and info stay as they were."""
    ctx = default_context()
    n, hb = 130, 130
    c = co.case("int_well", n, hb)
    A, b = c["A"], c["B"][0]
    wsb = lib.mm_chol_workspace_bytes(n)
    ws = workspace(n)
    big = torch.zeros(n * n + 1, dtype=torch.float64, device=DEV)
    big[:n * n] = dev(A).reshape(-1)
    odd = dev(A[:n - 1, :n - 1])
    Ad, bd = dev(A), dev(b)
    info = torch.full((1,), 777, dtype=torch.int32, device=DEV)
    ctx.sync()
    ctx.profile(1)
    try:
        calls = {
            "odd n": (lib.mm_chol_solve(ctx.h, ptr(odd), n - 1, ptr(bd), 1, hb, ptr(info), ptr(ws), wsb), MM_ERR_ARG),
            "odd n sym": (lib.mm_chol_solve_sym(ctx.h, ptr(odd), n - 1, ptr(bd), hb, 1, ptr(info), ptr(ws), wsb), MM_ERR_ARG),
            "A + 8 bytes": (lib.mm_chol_solve(ctx.h, big.data_ptr() + 8, n, ptr(bd), 1, hb, ptr(info), ptr(ws), wsb), MM_ERR_ARG),
            "A + 8 bytes sym": (lib.mm_chol_solve_sym(ctx.h, big.data_ptr() + 8, n, ptr(bd), hb, 1, ptr(info), ptr(ws), wsb),
                                MM_ERR_ARG),
            "workspace one byte short": (lib.mm_chol_solve(ctx.h, ptr(Ad), n, ptr(bd), 1, hb, ptr(info), ptr(ws), wsb - 1),
                                         MM_ERR_WORKSPACE),
            "workspace one byte short sym": (lib.mm_chol_solve_sym(ctx.h, ptr(Ad), n, ptr(bd), hb, 1, ptr(info), ptr(ws), wsb - 1),
                                             MM_ERR_WORKSPACE),
            "b NULL with nrhs 1": (lib.mm_chol_solve(ctx.h, ptr(Ad), n, None, 1, hb, ptr(info), ptr(ws), wsb), MM_ERR_ARG),
            "n = 0": (lib.mm_chol_solve(ctx.h, ptr(Ad), 0, ptr(bd), 1, 0, ptr(info), ptr(ws), wsb), 0),
            "n = 0 sym": (lib.mm_chol_solve_sym(ctx.h, ptr(Ad), 0, ptr(bd), 0, 1, ptr(info), ptr(ws), wsb), 0),
        }
        launched = ctx.profile_report()
    finally:
        ctx.profile(0)
    for name, (rc, want) in calls.items():
        assert rc == want, (name, rc, want)
    assert launched == {}, launched
    assert int(info) == 777 and (host(Ad) == A).all() and (host(bd) == b).all()
    # nrhs = 0 with b = NULL factors only
    info0, _, Lg = solve("chol", nan_upper(A), None, hb)
    assert info0 == 0
    rho = co.factor_residual(A, np.tril(Lg))
    print(f"\nG factor only {n}/{hb}: rho {rho:.3g}  rho/LAPACK {rho / c['rho_lapack']:.3g}")
    assert rho <= co.bar_factor_well(c["rho_lapack"])
    _, _, L1 = solve("chol", A, b, hb)
    assert (bits(np.tril(Lg)) == bits(np.tril(L1))).all()
