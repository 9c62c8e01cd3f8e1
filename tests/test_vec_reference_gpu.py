"""GPU: the trust-region vector layer (csrc/vec.hip) -- mm_multi_dot and the fused passes mm_trf_fused, ops 0-5 -- against
the exact CPU reference of oracle/vec_oracle.py at the edges of the launch geometry: slice boundaries, the 16-byte pair
path against the element-by-element path, every position of `split`.

Element outputs are compared bit for bit (ops 2 and 4: with every contraction the compiler may choose).  Every sum is
within (depth + 1) eps sum|a_i b_i| of the exact sum of the kernel's own element outputs, depth counted from the code
in vec_oracle.partition (tests/test_vec_reference_cpu.py shows on the CPU that the bound is attainable); the total
column is fl(camera + point).  Every operand and every output lies between NaN guards: a write next to an output
changes a guard, a read past an input turns a sum into NaN, and a non-finite value anywhere fails.

A NaN in g is dropped from op 0's maxima row by fmax; the solvers reject non-finite residuals before the first pass, so
that behaviour is left as it is and not tested here.

Run on the MI355X box:  python -m pytest tests/test_vec_reference_gpu.py -q -s
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

# ---- the shapes: the smallest at which the partition can go wrong, not workload sizes.  512 threads, twice that (one trip of
# the fused loop), the slice unit 2048, the first grids of 2 / 3 / 4 workgroups, and both sides of the 256-workgroup cap
# (524_288 = 256 * 2048), where ceil(n / grid) turns odd and the fused passes round it up.  (literals: the CPU test reads them)
N_SMALL = (1, 2, 3, 511, 512, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4097, 6145)      # every edge value of `split`
N_LARGE = (524_287, 524_288, 524_289, 524_291, 1_048_577)                                # split: 0, odd, even, n
N_LARGE_FEW = (524_287, 524_289)              # the large n of ops 1, 2, 4, 5 and of k = 2, 5
# (MM_VEC_GRID, two n): one workgroup that is also the last one; 2048 workgroups, whose partials take the last workgroup
# more than one trip (601 and 2048 workgroups; 4_194_307 = 2048 * 2048 + 3 is capped and has an odd ceil(n / grid))
GRID_CASES = ((1, (1025, 6145)), (2048, (1_228_801, 4_194_307)))
N_ALIGN = 4097                                # the slot-by-slot alignment test: 3 workgroups, odd, split = per = 1366

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from meatmodeler_amd import bundleAdjuster, ops, synth  # noqa: E402
from meatmodeler_amd._lib import MMError, default_context, lib  # noqa: E402
from oracle import vec_oracle as vo  # noqa: E402

DEV = torch.device("cuda", 0)
LD = np.longdouble
CAP = vo.grid_cap()                     # what the library read from MM_VEC_GRID (256 without it)
GUARD = 64                              # doubles of NaN before and after every operand and output
NAN_OUT, NAN_IN = 0x7FF8_0BAD_0BAD_0BAD, 0x7FF8_0123_4567_89AB      # guards of outputs / of inputs: a value computed from an
#                                                                       input's guard and stored next to an output differs from it
WS_BYTES = lib.mm_multi_dot_workspace_bytes()
N_OUT = (2, 2, 1, 3, 1, 1)
ROWS = (2, 3, 2, 6, 0, 0)               # result rows of an op (its sums and the maxima row)
# device scalars and step lengths: no round numbers
GH2, SC, WN2, P01, H01 = 3.712304111, -0.831700913, 0.019340771, (0.417300291, -0.229100377), (0.312700613, -1.709300847)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


class Worst:
    """check() of test_ba_reference_gpu.py, keeping the worst err / bound per name; report() prints them."""

    def __init__(self, group):
        self.group, self.worst = group, {}

    def check(self, name, got, ref, bound, where=()):
        """|got - ref| <= bound entrywise (bound 0: exactly equal).  A NaN or an infinity anywhere -- in what the kernel
        wrote, in the reference or in the bound -- fails."""
        got, ref = np.asarray(got).astype(LD), np.asarray(ref).astype(LD)
        assert got.shape == ref.shape and np.ndim(bound) <= ref.ndim, (name, where, got.shape, ref.shape)
        for what, a in (("kernel output", got), ("reference", ref), ("bound", np.asarray(bound))):
            assert np.isfinite(a).all(), (name, where, what, "is not finite", int((~np.isfinite(a)).sum()))
        bound = np.broadcast_to(np.asarray(bound).astype(LD), ref.shape)
        err = np.abs(got - ref)
        pos = bound > 0
        worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
        self.worst[name] = max(self.worst.get(name, 0.0), worst)
        bad = ~(err <= bound)
        assert not bad.any(), (name, where, int(bad.sum()), float(err[bad].max()), float(bound[bad].min()), worst)

    def report(self):
        for name, w in self.worst.items():
            print(f"  [{self.group}] {name:<30} worst err/bound {w:.3g}")


class Buf:
    """n doubles inside a larger allocation of NaNs: at least GUARD of them on either side; odd = True puts the
    first element at an address that is 8 modulo 16.  With data: an input, without: an output (all NaN until written)."""

    def __init__(self, n, data=None, odd=False):
        self.n, self.off = int(n), GUARD + (1 if odd else 0)
        self.nan = NAN_OUT if data is None else NAN_IN
        self.base = torch.full((self.n + 2 * GUARD + 2,), self.nan, dtype=torch.int64, device=DEV)
        assert self.base.data_ptr() % 16 == 0
        self.t = self.base.view(torch.float64)[self.off:self.off + self.n]
        self.ptr = self.base.data_ptr() + 8 * self.off          # (an empty view has no data_ptr of its own)
        assert self.ptr % 16 == (8 if odd else 0)
        if data is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(data, dtype=np.float64)))

    def guards_intact(self):
        b = self.base
        return bool((b[:self.off] == self.nan).all()) and bool((b[self.off + self.n:] == self.nan).all())

    def untouched(self):
        return bool((self.base == self.nan).all())


def new_ws():
    ws = torch.zeros(WS_BYTES, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    return ws


def _ptrs(bufs):
    return (C.c_void_p * max(len(bufs), 1))(*[b.ptr if isinstance(b, Buf) else b.data_ptr() for b in bufs])


def call_dot(ws, a, b, n, split, out, k=None, ws_bytes=None):
    ctx = default_context()
    k = len(a) if k is None else k
    ctx.check(lib.mm_multi_dot(ctx.h, k, _ptrs(a), _ptrs(b), int(n), int(split), out.ptr, ws.data_ptr(),
                               ws.numel() if ws_bytes is None else ws_bytes), "mm_multi_dot")


def call_fused(ws, op, ins, outs, scalars, h0, h1, n, split, res, ws_bytes=None):
    ctx = default_context()
    ctx.check(lib.mm_trf_fused(ctx.h, op, _ptrs(ins), _ptrs(outs), _ptrs(scalars) if scalars else None, float(h0), float(h1),
                               int(n), int(split), res.ptr, ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes),
              "mm_trf_fused")


def _splits(n):
    return vo.edge_splits(n, full=n in N_SMALL)


# ------------------------------------------------------------------------------------------------ A. mm_multi_dot

@functools.lru_cache(maxsize=4)
def _dot_data(n, k=8):
    rng = np.random.default_rng(77 + n)
    A = rng.normal(size=(k, n)) * 2.0 ** rng.integers(-6, 7, size=(k, n))
    return A, rng.normal(size=(k, n))


def _check_dot(W, A, B, n, runs, where):
    """runs: [(split, out [k,3])] of one set of operands: every column against the exact inner product of its part."""
    depth_bound = functools.partial(vo.sum_bound, n, "dot", cap=CAP)
    for q in range(A.shape[0]):
        sd = vo.SplitDot(A[q], B[q])
        for split, out in runs:
            exact, absd = sd.columns(split)
            W.check("multi_dot columns", out[q], exact, depth_bound(absd), where + (n, split, q))
            assert out[q, 2] == out[q, 0] + out[q, 1], (where, n, split, q)          # total = fl(camera + point)


def _run_dot(W, n, k, splits, A=None, B=None):
    """mm_multi_dot on the first k pairs at every split, operands alternating between 16-byte aligned and 8-byte offset
    addresses from call to call; every call twice (same bits), guards checked."""
    if A is None:
        A, B = _dot_data(n)
    A, B = A[:k], B[:k]
    ws = new_ws()
    copies = [([Buf(n, A[q], odd) for q in range(k)], [Buf(n, B[q], odd) for q in range(k)]) for odd in (False, True)]
    runs = []
    for j, split in enumerate(splits):
        a = [copies[(q + j) % 2][0][q] for q in range(k)]
        b = [copies[(q // 2 + j) % 2][1][q] for q in range(k)]
        out = Buf(3 * k)
        call_dot(ws, a, b, n, split, out)
        first = host(out.t).reshape(k, 3)
        assert out.guards_intact(), (n, k, split)
        out2 = Buf(3 * k)
        call_dot(ws, a, b, n, split, out2)
        assert np.array_equal(vo.bits(first), vo.bits(host(out2.t).reshape(k, 3))), (n, k, split)
        runs.append((split, first))
    assert int(ws[:4].view(torch.int32)) == 0
    _check_dot(W, A, B, n, runs, (k,))


@pytest.mark.parametrize("k", [1, 8])
def test_multi_dot_small_shapes(k):
    """Every small n of the table at every edge value of split, and one split past the end (all in the camera part)."""
    W = Worst("A")
    for n in N_SMALL:
        _run_dot(W, n, k, _splits(n) + [n + 5])
    W.report()


@pytest.mark.parametrize("n", N_LARGE)
@pytest.mark.parametrize("k", [1, 8])
def test_multi_dot_large_shapes(k, n):
    W = Worst("A")
    _run_dot(W, n, k, _splits(n))
    W.report()


@pytest.mark.parametrize("k", [2, 5])
def test_multi_dot_other_pair_counts(k):
    W = Worst("A")
    for n in (3, 1025, 4097) + N_LARGE_FEW[1:]:
        _run_dot(W, n, k, _splits(n)[1:4] if n in N_SMALL else _splits(n)[1:3])
    W.report()


def test_multi_dot_wrapper_chunks_eleven_pairs():
    """ops.MultiDot splits more than eight pairs over two launches on one workspace: rows in the order of the pairs."""
    W = Worst("A")
    rng = np.random.default_rng(5)
    n, k = 6145, 11
    A, B = rng.normal(size=(k, n)), rng.normal(size=(k, n)) * 2.0 ** rng.integers(-6, 7, size=(k, n))
    md = ops.MultiDot(DEV)
    ba, bb = [Buf(n, A[q], q % 2 == 1) for q in range(k)], [Buf(n, B[q], q % 3 == 1) for q in range(k)]
    runs = []
    for split in (0, 2049, 3072, n):
        out = md([(x.t, y.t) for x, y in zip(ba, bb)], split)
        assert tuple(out.shape) == (k, 3) and torch.equal(out, md([(x.t, y.t) for x, y in zip(ba, bb)], split))
        runs.append((split, host(out)))
    _check_dot(W, A, B, n, runs, ("wrapper",))
    W.report()


def test_multi_dot_bound_is_on_the_magnitudes_under_cancellation():
    """A sum that cancels to 1e-12 of its terms' magnitudes: the error is bounded by sum|a_i b_i|, not by the result."""
    W = Worst("A")
    rng = np.random.default_rng(9)
    m = 3072
    u, v = rng.normal(size=m), rng.normal(size=m)
    a, b = np.concatenate([u, u, [1.0]]), np.concatenate([v, -v, [3.1e-10]])
    perm = rng.permutation(a.size)
    a, b = a[perm], b[perm]
    n = a.size
    assert n == 6145 and vo.abs_dot(a, b) >= 1e12 * abs(vo.exact_dot(a, b)) > 0
    _run_dot(W, n, 1, [0, n], a[None], b[None])
    W.report()


# ------------------------------------------------------------------------------------------------ B. mm_trf_fused

@functools.lru_cache(maxsize=16)
def _vec_data(n):
    rng = np.random.default_rng(4242 + n)

    def r():
        return rng.normal(size=n) * 2.0 ** rng.integers(-6, 7, size=n)
    return dict(g=r(), si=rng.uniform(0.5, 2.0, size=n), q=r(), gh=r(), gn=r(), q1=r(), w=r(), x=r(), s1=r(), s2=r())


NANV = np.full(1, np.nan)          # stands for an empty operand (v with split = 0, dp with split = n): never read


def _fused_operands(op, d, split, p1_zero=False):
    """-> (inputs, device scalars, h0, h1) of an op on the data d."""
    n = d["si"].size
    if op == 0:
        return [d["g"], d["si"]], [], 0.0, 0.0
    if op == 1:
        return [d["q"][:split] if split else NANV, d["q"][split:] if split < n else NANV, d["si"], d["gh"]], [[GH2]], 0.0, 0.0
    if op == 2:
        return [d["gn"], d["q1"]], [[SC]], 0.0, 0.0
    if op == 3:
        return [d["w"], d["q1"], d["si"], d["gh"], d["x"]], [[WN2]], 0.0, 0.0
    if op == 4:
        return [d["x"], d["s1"], d["s2"]], [], H01[0], H01[1]
    # op 5 with p[1] == 0 must not read s2: it is all NaN here, and the result has to be finite
    return [d["x"], d["s1"], np.full(n, np.nan) if p1_zero else d["s2"]], [[P01[0], 0.0 if p1_zero else P01[1]]], 0.0, 0.0


def _sum_pairs(op, ins, outs):
    """The inner products an op reports, in row order, on its own element outputs."""
    o = outs
    return {0: lambda: [(o[0], o[0])], 1: lambda: [(o[1], o[0]), (o[0], o[0])], 2: lambda: [(o[0], o[0])],
            3: lambda: [(o[1], o[1]), (o[1], o[2]), (o[2], o[2]), (o[0], ins[3]), (ins[4], ins[4])]}.get(op, lambda: [])()


class FusedCase:
    """One (op, data) pair: the element reference and the exact products are formed once and shared by every split and
    layout (the element outputs do not depend on split; op 1 is handed the two halves of one vector q)."""

    def __init__(self, W, op, n, p1_zero=False, d=None):
        self.W, self.op, self.n, self.p1_zero = W, op, n, p1_zero
        self.d = d or _vec_data(n)
        ins, sc, h0, h1 = _fused_operands(op, self.d, n // 2, p1_zero)
        self.ref = vo.fused_reference(op, ins, sc, h0, h1, split=n // 2)
        self.sds = None           # [(a, b, SplitDot)] of the last outputs seen
        self.matched = {}         # candidate label -> calls in which it matched every element
        self.first_outs = None
        self.ws = new_ws()

    def run(self, split, odd_slot=None):
        op, n = self.op, self.n
        ins, sc, h0, h1 = _fused_operands(op, self.d, split, self.p1_zero)
        bi = [Buf(len(a), a, odd_slot == i) for i, a in enumerate(ins)]
        bo = [Buf(n, None, odd_slot == len(ins) + j) for j in range(N_OUT[op])]
        res = Buf(3 * max(ROWS[op], 1))
        sct = [dev(np.array(s)) for s in sc]
        call_fused(self.ws, op, bi, bo, sct, h0, h1, n, split, res)
        outs = [host(b.t) for b in bo]
        where = (op, n, split, odd_slot)
        assert all(b.guards_intact() for b in bo) and res.guards_intact(), where
        for b, a in zip(bi, ins):                                   # (and no input is written)
            assert b.guards_intact() and np.array_equal(vo.bits(host(b.t)), vo.bits(a)), where
        # element outputs, bit for bit
        for j, (got, cands) in enumerate(zip(outs, self.ref)):
            assert np.isfinite(got).all(), (where, j, "output is not finite")
            ok, counts = vo.match_candidates(got, cands)
            assert ok.all(), (where, j, int((~ok).sum()), int(np.flatnonzero(~ok)[0]), counts)
            for label, c in counts.items():
                if c == n:
                    self.matched[label] = self.matched.get(label, 0) + 1
        if self.first_outs is None:
            self.first_outs = outs
        elif op in (0, 1, 3, 5):      # one value per element whatever the path: aligned pairs or element by element
            assert all(np.array_equal(vo.bits(a), vo.bits(b)) for a, b in zip(outs, self.first_outs)), where
        rows = host(res.t).reshape(-1, 3)
        if ROWS[op] == 0:
            assert res.untouched(), where
            assert int(self.ws[:4].view(torch.int32)) == 0
            return outs, rows
        # sums: the accumulation of the kernel's own outputs
        pairs = _sum_pairs(op, ins, outs)
        if self.sds is None or not all(np.array_equal(a, c[0]) and np.array_equal(b, c[1]) for (a, b), c in zip(pairs, self.sds)):
            self.sds = [(a, b, vo.SplitDot(a, b)) for a, b in pairs]
        for r, (_, _, sd) in enumerate(self.sds):
            exact, absd = sd.columns(split)
            self.W.check(f"op {op} sums", rows[r], exact, vo.sum_bound(n, "fused", absd, CAP), where + (r,))
            assert rows[r, 2] == rows[r, 0] + rows[r, 1], (where, r)
        if op == 0:
            g = np.abs(ins[0])
            want = [g[:split].max(initial=0.0), g[split:].max(initial=0.0), g.max(initial=0.0)]
            assert rows[1].tolist() == want, (where, rows[1].tolist(), want)
        assert int(self.ws[:4].view(torch.int32)) == 0
        return outs, rows

    def report(self):
        if self.op in (2, 4):
            print(f"  [B] op {self.op} n {self.n}: element outputs equal {sorted(self.matched.items())}")


def _variants(op):
    return (False, True) if op == 5 else (False,)


@pytest.mark.parametrize("op", [0, 1, 2, 3, 4, 5])
def test_fused_small_shapes(op):
    """Every small n at every edge value of split, all operands 16-byte aligned: an even split takes the 16-byte pair path
    (with the last element of an odd slice on its own), an odd split the element-by-element path."""
    W = Worst("B")
    paths = set()
    for n in N_SMALL:
        for p1_zero in _variants(op):
            case = FusedCase(W, op, n, p1_zero)
            for split in _splits(n):
                case.run(split)
                paths.add(split % 2)
            if n == N_SMALL[-1]:
                case.report()
    assert paths == {0, 1}
    W.report()


@pytest.mark.parametrize("op,n", [(op, n) for op in (0, 3) for n in N_LARGE] + [(op, n) for op in (1, 2, 4, 5) for n in N_LARGE_FEW])
def test_fused_large_shapes(op, n):
    """Both sides of the grid cap: 256 workgroups whose slices are 2048 (even) or 2049 -> 2050 (rounded) long."""
    W = Worst("B")
    for p1_zero in _variants(op):
        case = FusedCase(W, op, n, p1_zero)
        splits = _splits(n)
        assert {s % 2 for s in splits} == {0, 1}
        for split in splits:
            case.run(split)
        case.report()
    W.report()


@pytest.mark.parametrize("op", [0, 1, 2, 3, 4, 5])
def test_fused_every_operand_slot_at_an_8_byte_offset(op):
    """One operand at a time -- every input, every output -- sits at an address that is 8 modulo 16, with an even split: the
    launch must leave the 16-byte path for that slot alone, and ops 0, 1, 3, 5 must give the bits of the aligned layout."""
    W = Worst("B")
    n = N_ALIGN
    split = vo.partition(n, "fused", vo.GRID_CAP)["per"]
    assert split % 2 == 0 and 0 < split < n
    for p1_zero in _variants(op):
        case = FusedCase(W, op, n, p1_zero)
        case.run(split)                                   # aligned: what the others are compared with
        n_slots = len(_fused_operands(op, case.d, split)[0]) + N_OUT[op]
        for slot in range(n_slots):
            case.run(split, odd_slot=slot)
        case.report()
    W.report()


@pytest.mark.parametrize("split", [1366, 2049])
def test_op0_maxima_at_the_ends_and_on_negative_entries(split):
    """max |g| per part: in the first element, in the last, next to the split, and belonging to a negative entry."""
    n = N_ALIGN
    base = dict(_vec_data(n))
    W = Worst("B")
    for marks in ({0: -1.0e3, n - 1: 2.0e3}, {split - 1: 5.0e2, split: -7.0e2}, {0: 3.0e3, split: 4.0e3}, {n - 1: -9.0e3}):
        g = base["g"].copy()
        for i, v in marks.items():
            g[i] = v
        _, rows = FusedCase(W, 0, n, d=dict(base, g=g)).run(split)
        want = [np.abs(g[:split]).max(), np.abs(g[split:]).max(), np.abs(g).max()]
        assert rows[1].tolist() == want and want[2] == max(abs(v) for v in marks.values())
        assert all(abs(v) in want for v in marks.values())          # (every marked entry is the maximum of its part)


def test_op5_skips_s2_when_p1_is_zero():
    """p[1] == 0: the output is finite although s2 is all NaN and equals fma(p0, s1, x); p[1] != 0: the two-fma chain."""
    W = Worst("B")
    for n in (3, 1025, 4097):
        d = _vec_data(n)
        for split in (0, 1, n // 2 & ~1, n):
            one, _ = FusedCase(W, 5, n, True).run(split)
            two, _ = FusedCase(W, 5, n, False).run(split)
            assert np.array_equal(vo.bits(one[0]), vo.bits(vo.fma(P01[0], d["s1"], d["x"])))
            assert np.array_equal(vo.bits(two[0]), vo.bits(vo.fma(P01[1], d["s2"], one[0])))
            assert not np.array_equal(one[0], two[0])


def test_argument_errors_touch_nothing():
    """split > n (fused), k = 0, k = 9, a workspace at a 128-byte offset, a short workspace: MMError with the documented
    code (MM_ERR_ARG = -1, MM_ERR_WORKSPACE = -3) before the device is touched -- outputs and workspace stay as they were."""
    n = 1000
    d = _vec_data(1025)
    raw = torch.full((WS_BYTES + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 256 == 0
    good, off128 = raw[:WS_BYTES], raw[128:128 + WS_BYTES]
    a, b = Buf(n, d["g"][:n]), Buf(n, d["si"][:n])
    o0, o1, res = Buf(n), Buf(n), Buf(6)

    def expect(code, fn, *args, **kw):
        with pytest.raises(MMError, match=rf"failed \({code}\)"):
            fn(*args, **kw)
        assert o0.untouched() and o1.untouched() and res.untouched()
        assert bool((raw == 0xA5).all())

    expect(-1, call_fused, good, 0, [a, b], [o0, o1], [], 0.0, 0.0, n, n + 1, res)
    expect(-1, call_dot, good, [a], [b], n, 0, res, k=0)
    expect(-1, call_dot, good, [a] * 9, [b] * 9, n, 0, res, k=9)
    expect(-3, call_dot, off128, [a], [b], n, 0, res)
    expect(-3, call_fused, off128, 0, [a, b], [o0, o1], [], 0.0, 0.0, n, 10, res)
    expect(-3, call_dot, good, [a], [b], n, 0, res, ws_bytes=WS_BYTES - 1)
    expect(-3, call_fused, good, 0, [a, b], [o0, o1], [], 0.0, 0.0, n, 10, res, ws_bytes=WS_BYTES - 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ C. the workspace contract

def test_workspace_resets_itself_across_kernels_and_grids():
    """One workspace, zero-filled once, through 24 calls that alternate between both kernels, grids of 1, 2 and 256
    workgroups and the passes that return without touching the counter: every result has the bits the same call gives on
    a fresh zero-filled workspace, and the counter word reads 0 at the end."""
    big, mid = 524_289, 2049
    A, B = _dot_data(big)
    db, dm, d1 = _vec_data(big), _vec_data(mid), _vec_data(1)
    dots8 = ([Buf(big, A[q]) for q in range(8)], [Buf(big, B[q]) for q in range(8)])
    dot1 = ([Buf(mid, dm["g"])], [Buf(mid, dm["w"])])

    def fused(op, d, split):
        ins, sc, h0, h1 = _fused_operands(op, d, split)
        n = d["si"].size
        bi, sct = [Buf(len(a), a) for a in ins], [dev(np.array(s)) for s in sc]

        def go(ws):
            bo, res = [Buf(n) for _ in range(N_OUT[op])], Buf(3 * max(ROWS[op], 1))
            call_fused(ws, op, bi, bo, sct, h0, h1, n, split, res)
            got = [host(b.t) for b in bo] + [host(res.t)[:3 * ROWS[op]]]
            assert all(np.isfinite(x).all() for x in got) and all(b.guards_intact() for b in bo + [res])
            return got
        return go

    def dot(ab, n, split):
        def go(ws):
            out = Buf(3 * len(ab[0]))
            call_dot(ws, ab[0], ab[1], n, split, out)
            got = host(out.t)
            assert np.isfinite(got).all() and out.guards_intact()
            return [got]
        return go

    calls = [dot(dots8, big, 3001), fused(3, d1, 1), dot(dot1, mid, 1024), fused(4, dm, 6), fused(5, dm, 7), fused(0, db, 262_144)]
    fresh = [go(new_ws()) for go in calls]
    ws = new_ws()
    count = 0
    for rnd in range(4):
        for go, want in zip(calls[rnd % 2:] + calls[:rnd % 2], fresh[rnd % 2:] + fresh[:rnd % 2]):
            got = go(ws)
            assert all(np.array_equal(vo.bits(x), vo.bits(y)) for x, y in zip(got, want)), (rnd, count)
            count += 1
    assert count >= 20 and int(ws[:4].view(torch.int32)) == 0


# ------------------------------------------------------------------------------------- D. grid caps outside the default

def _grid_child():
    """Runs in a fresh interpreter with MM_VEC_GRID set (the library reads it once per process): mm_multi_dot with k = 8
    and fused ops 0 and 3 at the cap's two n, checked like everything above with the partition told the cap."""
    cap = int(os.environ["MM_VEC_GRID"])
    assert CAP == cap
    ns = dict(GRID_CASES)[cap]
    W = Worst("D")
    for n in ns:
        assert vo.partition(n, "dot", cap)["grid"] == min(-(-n // 2048), cap)
        splits = vo.edge_splits(n, full=False)[1:3]
        _run_dot(W, n, 8, splits)
        for op in (0, 3):
            case = FusedCase(W, op, n)
            for split in splits:
                case.run(split)
    W.report()
    print(f"ok MM_VEC_GRID={cap} n={ns}")


@pytest.mark.parametrize("cap", [c for c, _ in GRID_CASES])
def test_grid_caps_outside_the_default(cap):
    """MM_VEC_GRID=1: the only workgroup is also the last one.  MM_VEC_GRID=2048: the last workgroup needs more than one
    trip over the partials (601 and 2048 of them)."""
    assert all(vo.partition(n, "fused", cap)["grid"] > (512 if cap > 1 else 0) for n in dict(GRID_CASES)[cap])
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {here!r}); import test_vec_reference_gpu as t; t._grid_child()"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MM_VEC_GRID=str(cap)), capture_output=True, text=True,
                       timeout=300, cwd=os.path.dirname(here))
    print(r.stdout, end="")
    assert r.returncode == 0 and f"ok MM_VEC_GRID={cap}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------- E. odd vector length inside the solvers

def test_solvers_agree_on_an_odd_vector_length():
    """n = 6 F + 3 P is odd when P is: the last element of the last slice goes through the element path in every pass.  The
    lock-step solve equals the one-problem solve, and the Python-sequenced loop the library loop, bit for bit."""
    if os.environ.get("MM_CHOL_FUSED") == "0":
        pytest.skip("MM_CHOL_FUSED=0 forces the launch-per-column factorisation: this test is about the single launch")
    if os.environ.get("MM_TRF_DRIVER", "library") != "library":
        pytest.skip("MM_TRF_DRIVER selects the Python-sequenced loop: this test is about the loop inside the library")
    ctx = default_context()
    probs, x0 = [], []
    for F, P, L, seed, noise in [(24, 701, 6, 11, 0.5), (31, 333, 5, 12, 1.0)]:
        assert (6 * F + 3 * P) % 2 == 1
        pr = synth.make_ba_problem(F, P, L, seed=seed)
        obs = pr["obs"] + np.random.default_rng(seed).normal(0, noise, pr["obs"].shape)
        with np.errstate(all="ignore"):
            cams0 = bundleAdjuster.frameParameters(pr["ext"]).reshape(F, 6)
        probs.append(ops.BADevice(pr["K"], pr["fi"], pr["pi"], obs, F, P, DEV, ctx))
        x0.append((dev(cams0), dev(pr["pts0"].copy())))
    tol = (1e-6, 1e-8, 1e-8)
    alone = []
    for pb, (c0, p0) in zip(probs, x0):
        c, p_ = c0.clone(), p0.clone()
        rep, _ = pb.trf_solve(c, p_, *tol)
        assert rep.nfev > 2 and rep.status > 0
        alone.append((c, p_, rep))
    cb, pbs = [c.clone() for c, _ in x0], [p_.clone() for _, p_ in x0]
    reps, _ = ops.trf_solve_batched(probs, cb, pbs, *tol, ctx=ctx)
    for (c, p_, rep), c2, p2, rep2 in zip(alone, cb, pbs, reps):
        assert (rep.nfev, rep.njev, rep.status) == (rep2.nfev, rep2.njev, rep2.status)
        assert rep.cost == rep2.cost and rep.optimality == rep2.optimality
        assert torch.equal(c, c2) and torch.equal(p_, p2)
    for pb, (c0, p0), (c, p_, rep) in zip(probs, x0, alone):
        pb.overlap = False
        res = {drv: bundleAdjuster.SchurTRF(pb, driver=drv).solve(c0.clone(), p0.clone(), *tol) for drv in ("python", "library")}
        a, b = res["python"], res["library"]
        assert "library" in b.host_segments_ms and "library" not in a.host_segments_ms
        assert (a.nfev, a.njev, a.status, a.iterations) == (b.nfev, b.njev, b.status, b.iterations)
        assert a.cost == b.cost and a.optimality == b.optimality
        assert torch.equal(a.cams, b.cams) and torch.equal(a.pts, b.pts)
        assert torch.equal(b.cams.reshape(c.shape), c) and torch.equal(b.pts.reshape(p_.shape), p_) and b.nfev == rep.nfev
