"""The decision machine of the trust-region loops exists twice: csrc/trf_decide.h (asked by mm_ba_trf / _dist / _fixed and
by the lock-step batch) and bundleAdjuster._TrfDecide (asked by the two loops sequenced from Python).  Here the same boards
go through both -- the header compiled alone with g++ behind tests/trf_decide_replay.cpp -- and the outcome and the full
state after EVERY call, the table rows and the report must be equal with == (NaN equals NaN).  SciPy's own
update_tr_radius / check_termination are asked as a third voice on Delta and the termination code of every trial step."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.optimize._lsq import common

from meatmodeler_amd import bundleAdjuster as ba
from meatmodeler_amd._lib import TrfParams, TrfRow, TrfReport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("outcome", "Delta", "cost", "cost0", "x_norm", "step_norm", "actual", "g_norm", "min_damping", "reg", "nfev", "njev",
          "iteration", "termination", "attempt", "max_nfev", "accepted", "n_log")
NAMES = {getattr(ba._TrfDecide, k): k for k in ("BODY", "TRIAL", "FINAL", "DONE", "RETRY", "USABLE", "ABANDONED", "INDEFINITE")}
T = ba._TrfDecide
INF, NAN = float("inf"), float("nan")


def same(a, b):
    return a == b or (a != a and b != b)


def all_same(a, b):
    """Nested tuples / lists of numbers, NaN equal to NaN."""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(all_same(x, y) for x, y in zip(a, b))
    return same(a, b)


def board(info=0, reg=1e-3, g=1.0, xx=4.0, pred=1.0, sh=1.0, sn=1.0, cost2=0.0):
    """What a driver reads after a trial step: info, damping used, |g|_inf, |x|^2, predicted, |p|, step norm, 2 * cost."""
    return [float(info), reg, g, xx, pred, sh, sn, cost2]


class Replay:
    """The driver of tests/trf_decide_replay.cpp over the Python machine, one board at a time (so that a scenario can look at
    the state before it writes the next board).  Every call of the machine leaves a record; every board is kept."""

    def __init__(self, cost0=10.0, xx_scaled=4.0, n=10, ftol=1e-4, xtol=1e-8, gtol=1e-8, max_nfev=0, min_damping=0.0):
        self.args = (cost0, xx_scaled, n)
        self.prm = dict(ftol=ftol, xtol=xtol, gtol=gtol, min_damping=min_damping, max_nfev=max_nfev)
        self.log, self.boards, self.records = [], [], []
        self.td = ba._TrfDecide(cost0, xx_scaled, n, ftol, xtol, gtol, max_nfev, min_damping, log=self.log)
        self.state = self._note(self.td.begin())

    def _note(self, outcome):
        td = self.td
        self.records.append((outcome, td.Delta, td.cost, td.cost0, td.x_norm, td.step_norm, td.actual, td.g_norm, td.min_damping,
                             td.reg, td.nfev, td.njev, td.iteration, -100 if td.termination is None else td.termination,
                             td.attempt, td.max_nfev, int(td.accepted), td.n_log))
        return outcome

    @property
    def alive(self):
        return self.state not in (T.DONE, T.INDEFINITE)

    def outcomes(self):
        return [NAMES[r[0]] for r in self.records]

    def feed(self, b):
        assert self.alive
        td = self.td
        self.boards.append(b)
        if self.state == T.FINAL:
            self.state = self._note(td.on_final(b[2]))
            return self.state
        if self.state != T.TRIAL:
            self.state = self._note(td.on_solve(int(b[0]), b[1], b[2], b[3]))
            if self.state != T.USABLE:
                return self.state
        # SciPy on this trial step, from the state before it
        Delta, cost_new = td.Delta, 0.5 * b[7]
        want_Delta, want_term = 0.25 * b[5], None
        if np.isfinite(cost_new):
            actual = td.cost - cost_new
            Delta_sp, ratio = common.update_tr_radius(Delta, actual, b[4], b[5], b[5] > 0.95 * Delta)
            want_term = common.check_termination(actual, td.cost, b[6], td.x_norm, ratio, self.prm["ftol"], self.prm["xtol"])
            want_Delta = Delta_sp if want_term is None else Delta
        self.state = self._note(td.on_trial(b[4], b[5], b[6], b[7]))
        assert same(td.Delta, want_Delta) and td.termination == want_term, (b, td.Delta, want_Delta, td.termination, want_term)
        return self.state


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("trf_decide") / "libtrf_decide_replay.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "meatmodeler_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "trf_decide_replay.cpp")])
    L = C.CDLL(so)
    L.trf_decide_replay.restype = C.c_int
    L.trf_decide_replay.argtypes = [C.POINTER(TrfParams), C.c_double, C.c_double, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_int, C.POINTER(TrfRow), C.c_int, C.POINTER(TrfReport)]
    return L


def assert_cxx_equals(shim, rp):
    """The boards of a finished Python replay through the C++ machine: every record, row and report field equal."""
    prm = TrfParams(**rp.prm)
    boards = np.ascontiguousarray(np.array(rp.boards, np.float64).reshape(-1, 8))
    cap = 2 * len(boards) + 2
    records = np.full((cap, len(FIELDS)), -7.0)
    rows = (TrfRow * 4096)()
    rep = TrfReport()
    calls = shim.trf_decide_replay(C.byref(prm), *rp.args, boards.ctypes.data, len(boards), records.ctypes.data, cap, rows, 4096,
                                   C.byref(rep))
    assert calls == len(rp.records), (calls, len(rp.records), rp.outcomes())
    for k, (want, got) in enumerate(zip(rp.records, records[:calls].tolist())):
        for name, a, b in zip(FIELDS, want, got):
            assert same(float(a), b), (k, name, a, b, rp.outcomes()[:k + 1])
    td = rp.td
    assert rep.log_rows == td.n_log == len(rp.log)
    for k, want in enumerate(rp.log):
        r = rows[k]
        got = (r.iteration, r.nfev, r.cost, r.reduction, r.step_norm, r.optimality)
        assert all(same(a, b) for a, b in zip(want, got)), (k, want, got)
    want = (td.cost0, td.cost, td.g_norm, td.min_damping, td.nfev, td.njev, td.status, td.iteration)
    got = (rep.cost0, rep.cost, rep.optimality, rep.min_damping, rep.nfev, rep.njev, rep.status, rep.iterations)
    assert all(same(a, b) for a, b in zip(want, got)), (want, got)


def test_scripted_decisions_python_equals_cxx(shim):
    """Every named decision, reached on purpose (cost 10 at the start, so 2 * cost = 20; Delta0 = 2)."""
    done = []

    def close(rp):
        assert_cxx_equals(shim, rp)
        done.append(rp)
        return rp

    # max_nfev = 1: nothing but the final gradient pass
    rp = Replay(max_nfev=1)
    assert rp.state == T.FINAL and rp.feed(board(g=0.5)) == T.DONE
    td = close(rp).td
    assert (td.nfev, td.njev, td.status, td.iteration, td.g_norm, td.cost, td.n_log) == (1, 1, 0, 0, 0.5, 10.0, 1)
    # Delta0 = 0 -> 1;  max_nfev <= 0 -> 100 n;  min_damping <= 0 -> 1e-9
    rp = Replay(xx_scaled=0.0, n=7)
    assert (rp.td.Delta, rp.td.max_nfev, rp.td.min_damping, rp.state) == (1.0, 700, 1e-9, T.BODY)
    close(rp)
    assert Replay(xx_scaled=9.0, max_nfev=5, min_damping=1e-6).td.__dict__.items() >= dict(Delta=3.0, max_nfev=5, min_damping=1e-6).items()
    # gtol on the first board: the trial step that came with it is dropped
    rp = Replay(gtol=1e-3)
    assert rp.feed(board(g=1e-4, cost2=2.0)) == T.DONE
    td = close(rp).td
    assert (td.nfev, td.njev, td.status, td.iteration, td.cost, td.n_log) == (1, 1, 1, 0, 10.0, 1) and np.isnan(td.actual)
    # ftol (2), xtol (3), both (4): an accepted step that ends the solve, then the final pass
    for ftol, xtol, status in ((1e-2, 1e-12, 2), (1e-12, 1e-2, 3), (1e-2, 1e-2, 4)):
        rp = Replay(ftol=ftol, xtol=xtol)
        assert rp.feed(board(pred=0.01, sn=1e-3, cost2=2 * 9.99)) == T.FINAL and rp.td.accepted
        assert rp.td.Delta == 2.0      # (the radius is not updated by a terminating step)
        assert rp.feed(board(g=0.25)) == T.DONE
        td = close(rp).td
        assert (td.nfev, td.njev, td.status, td.iteration, td.cost, td.g_norm) == (2, 2, status, 1, 9.99, 0.25)
        assert rp.outcomes() == ["BODY", "USABLE", "FINAL", "DONE"]
    # predicted = 0 with actual = 0: the ratio is 1 (at the bound the radius doubles; a ratio of 0 would shrink it)
    rp = Replay(ftol=0.0, xtol=0.0)
    assert rp.feed(board(pred=0.0, sh=1.95, cost2=20.0)) == T.TRIAL
    assert (rp.td.Delta, rp.td.actual, rp.td.nfev, rp.td.iteration) == (4.0, 0.0, 2, 0)
    close(rp)
    # ratio < 0.25 shrinks Delta to 0.25 * step_h_norm (the step is still accepted)
    rp = Replay(ftol=0.0, xtol=0.0)
    assert rp.feed(board(pred=1.0, sh=1.5, cost2=2 * 9.9)) == T.BODY
    assert (rp.td.Delta, rp.td.accepted, rp.td.cost, rp.td.njev, rp.td.iteration) == (0.375, True, 9.9, 2, 1)
    close(rp)
    # ratio > 0.75 at the bound doubles Delta -- and not inside it
    for sh, want in ((1.99, 4.0), (1.5, 2.0)):
        rp = Replay(ftol=0.0, xtol=0.0)
        assert rp.feed(board(pred=1.0, sh=sh, cost2=2 * 9.1)) == T.BODY and rp.td.Delta == want
        close(rp)
    # rejected steps until max_nfev is hit inside the trial loop: the iteration counts, then the final pass, status 0
    rp = Replay(max_nfev=4)
    worse = board(pred=1.0, sh=1.0, sn=0.7, cost2=22.0)
    assert [rp.feed(worse), rp.feed(worse), rp.feed(worse)] == [T.TRIAL, T.TRIAL, T.FINAL]
    assert (rp.td.nfev, rp.td.iteration, rp.td.step_norm, rp.td.actual, rp.td.accepted, rp.td.njev) == (4, 1, 0.0, 0.0, False, 1)
    assert rp.feed(board(g=3.0)) == T.DONE
    td = close(rp).td
    assert (td.status, td.cost, td.n_log) == (0, 10.0, 2) and rp.log[-1] == (1, 4, 10.0, 0.0, 0.0, 3.0)
    # a non-finite trial cost: Delta = 0.25 * step_h_norm, nothing else moves, another trial step
    for bad in (INF, -INF, NAN):
        rp = Replay()
        assert rp.feed(board(sh=1.2, cost2=bad)) == T.TRIAL
        assert (rp.td.Delta, rp.td.actual, rp.td.nfev, rp.td.cost, rp.td.termination) == (0.25 * 1.2, -1.0, 2, 10.0, None)
        assert rp.feed(board(sh=0.3, cost2=18.0)) == T.BODY and rp.td.accepted
        close(rp)
    # not positive definite with the damping above the floor: the floor stays; at the floor: x100, and it stays raised
    rp = Replay()
    assert rp.feed(board(info=3, reg=1e-3)) == T.RETRY and (rp.td.min_damping, rp.td.reg, rp.td.attempt) == (1e-9, 0.1, 1)
    assert rp.feed(board(info=3, reg=1e-9)) == T.RETRY and (rp.td.min_damping, rp.td.reg, rp.td.attempt) == (1e-9 * 100.0, 1e-9 * 100.0, 2)
    assert rp.feed(board(info=0, cost2=18.0)) == T.BODY and (rp.td.min_damping, rp.td.attempt, rp.td.nfev) == (1e-9 * 100.0, 0, 2)
    close(rp)
    # five failures, a success, later five more: the count starts again, no INDEFINITE
    rp = Replay(ftol=0.0, xtol=0.0)
    for _ in range(2):
        assert [rp.feed(board(info=1, reg=0.5)) for _ in range(5)] == [T.RETRY] * 5
        assert rp.feed(board(info=0, cost2=2 * 0.9 * rp.td.cost, pred=0.1 * rp.td.cost)) == T.BODY and rp.td.attempt == 0
    assert "INDEFINITE" not in close(rp).outcomes() and rp.td.iteration == 2
    # six in a row: INDEFINITE at the sixth
    rp = Replay()
    assert [rp.feed(board(info=2, reg=0.5)) for _ in range(6)] == [T.RETRY] * 5 + [T.INDEFINITE]
    assert not rp.alive and rp.td.nfev == 1
    close(rp)
    # an abandoned factorisation leaves no trace: the same board with info 0 behaves as if the -1 was never seen
    b = board(info=-1, reg=2e-3, g=0.7, xx=5.0, pred=2.0, sh=1.0, sn=0.4, cost2=17.0)
    rp, plain = Replay(), Replay()
    before = rp.records[-1][1:]
    assert rp.feed(b) == T.ABANDONED and all_same(rp.records[-1][1:], before)
    assert rp.feed([0.0] + b[1:]) == plain.feed([0.0] + b[1:]) == T.BODY
    assert all_same(rp.records[-2:], plain.records[-2:]) and all_same(rp.log, plain.log) and len(rp.log) == 1
    close(rp)
    # and the scenarios did reach what they are named after
    seen = {o for rp in done for o in rp.outcomes()}
    assert seen == set(NAMES.values())
    assert {rp.td.termination for rp in done} >= {None, 1, 2, 3, 4}


def test_random_walk_python_equals_cxx(shim):
    """250 seeded problems, boards written while looking at the Python machine's state so that accepted, rejected,
    terminating, non-finite, indefinite and abandoned steps all keep occurring; whole traces compared."""
    rng = np.random.default_rng(20240607)
    seen, statuses = set(), set()
    for _ in range(250):
        rp = Replay(cost0=10.0 ** rng.uniform(-3, 3), xx_scaled=float(rng.choice([0.0, rng.uniform(0, 50)])), n=int(rng.integers(3, 50)),
                    ftol=float(rng.choice([1e-2, 1e-4, 1e-8])), xtol=float(rng.choice([1e-3, 1e-8])), gtol=float(rng.choice([1e-3, 1e-8])),
                    max_nfev=int(rng.choice([0, 1, 2, 5, 30])), min_damping=float(rng.choice([0.0, 1e-9, 1e-6])))
        while rp.alive and len(rp.boards) < 80:
            td = rp.td
            info = int(rng.choice([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 5, 77, -1, 0]))
            reg = float(rng.choice([td.min_damping, td.min_damping * (1.0 + 1e-13), td.min_damping * (1.0 + 1e-11),
                                    td.reg if td.reg > 0 else 1e-4, 10.0 ** rng.uniform(-9, -2)]))
            pred = float(rng.choice([0.0, -1e-3 * td.cost, td.cost * 10.0 ** rng.uniform(-7, -0.1)], p=[0.05, 0.05, 0.9]))
            actual = pred * float(rng.choice([-1.0, 0.0, 0.1, 0.24, 0.26, 0.5, 0.76, 1.0, 1.3]))
            cost2 = float(rng.choice([2.0 * (td.cost - actual), INF, NAN], p=[0.94, 0.03, 0.03]))
            sh = td.Delta * float(rng.choice([0.2, 0.949, 0.951, 1.0]))
            rp.feed(board(info, reg, 10.0 ** rng.uniform(-9, 2), rng.uniform(0, 100), pred, sh, sh * 10.0 ** rng.uniform(-7, 0), cost2))
        assert_cxx_equals(shim, rp)
        seen.update(rp.outcomes())
        if not rp.alive and rp.state == T.DONE:
            statuses.add(rp.td.status)
    assert seen >= set(NAMES.values()) - {"INDEFINITE"}
    assert statuses == {0, 1, 2, 3, 4}
