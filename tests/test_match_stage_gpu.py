"""GPU: the match stage as one native call (mm_bf_match_ratio_batched) against the CPU oracle and, byte for byte, against
the two calls it replaces (mm_bf_knn2_batched + mm_ratio_filter_batched).  Everything here is integer data: equality is
exact.

Run on the MI355X box:  python -m pytest tests/test_match_stage_gpu.py -m gpu -q
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from meatmodeler_amd import ops  # noqa: E402
from oracle import orb_oracle as oo  # noqa: E402

DEV = torch.device("cuda", 0)
CAP = 300                                   # 9 tiles of 32 train rows + 12: the last tile is partial at nt = nt_cap
THRESHOLD = 0.75


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def flipped(row, bits):
    """`row` (32 bytes) with the given bit positions inverted."""
    mask = np.zeros(256, np.uint8)
    mask[np.asarray(bits, np.int64)] = 1
    return row ^ np.packbits(mask, bitorder="little")


def ragged_batch():
    """Nine pairs (one more than a group of eight) at cap 300 whose counts cover nq in {0, 1, 255, 256, 257, 300} and nt in
    {0, 1, 31, 32, 33, 64, 65, 300}, with planted rows in pair 0 (300 x 300) and pair 8 (257 x 65).  Random rows lie
    ~128 +- 8 bits from everything else, so the planted distances (0 .. 40) are the two smallest of their queries."""
    rng = np.random.default_rng(2024)
    n_pairs = 9
    q = rng.integers(0, 256, (n_pairs, CAP, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (n_pairs, CAP, 32), dtype=np.uint8)
    nq = np.array([300, 0, 1, 255, 256, 257, 300, 300, 257], np.int32)
    nt = np.array([300, 300, 0, 1, 31, 32, 33, 64, 65], np.int32)
    bits = rng.permutation(256)
    want = {}                               # (pair, query) -> train index of the match, or -1
    # duplicate train rows: the best is the lowest index, the second its copy at the same distance -> never a match
    t[0, 70:75] = t[0, 3]
    q[0, 5] = flipped(t[0, 3], bits[:4])
    want[(0, 5)] = -1
    # best and second best in the same 32-row tile (rows 40 and 45), d = 10 and 40
    q[0, 10] = flipped(t[0, 40], bits[:10])
    t[0, 45] = flipped(t[0, 40], bits[10:40])
    want[(0, 10)] = 40
    # ... and in different tiles (rows 100 and 200)
    q[0, 11] = flipped(t[0, 100], bits[:10])
    t[0, 200] = flipped(t[0, 100], bits[10:40])
    want[(0, 11)] = 100
    # the ratio test at its edge, d1 = 40 -> 0.75 d1 = 30: d0 = 29 passes by one distance unit, d0 = 30 fails by one
    t[0, 231] = flipped(t[0, 230], bits[40:51])          # 11 bits from row 230
    q[0, 20] = flipped(t[0, 230], bits[:29])             # d(row 230) = 29, d(row 231) = 40
    want[(0, 20)] = 230
    t[0, 261] = flipped(t[0, 260], bits[40:50])          # 10 bits from row 260
    q[0, 21] = flipped(t[0, 260], bits[:30])             # d(row 260) = 30, d(row 261) = 40
    want[(0, 21)] = -1
    # the same edge in the ninth pair (the padded group), second best in the partial third tile (row 64 of 65)
    t[8, 64] = flipped(t[8, 2], bits[40:51])
    q[8, 256] = flipped(t[8, 2], bits[:29])
    want[(8, 256)] = 2
    q[8, 0] = flipped(t[8, 5], bits[:30])                # d(row 5) = 30, d(row 33) = 40: best and second in two tiles
    t[8, 33] = flipped(t[8, 5], bits[40:50])
    want[(8, 0)] = -1
    return q, t, nq, nt, want


@pytest.fixture(scope="module")
def batch():
    q, t, nq, nt, want = ragged_batch()
    oracle = []
    for p in range(len(nq)):
        io, do = oo.bf_knn2(q[p, :nq[p]], t[p, :nt[p]])
        oracle.append(oo.ratio_filter(io, do, THRESHOLD))
    for (p, qi), ti in want.items():        # the plants are what they were meant to be
        hit = oracle[p][oracle[p][:, 0] == qi]
        assert (len(hit) == 0) if ti < 0 else (len(hit) == 1 and hit[0, 1] == ti), (p, qi, ti, hit)
    return dict(q=dev(q), t=dev(t), nq=dev(nq), nt=dev(nt), oracle=oracle)


@pytest.mark.parametrize("variant", ["314", "114"])
def test_match_ratio_against_oracle(variant, batch, monkeypatch):
    monkeypatch.setenv("MM_BF_VARIANT", variant)
    pairs, m = ops.bf_match_ratio_batched(batch["q"], batch["t"], batch["nq"], batch["nt"], THRESHOLD)
    assert pairs.shape == (9, CAP, 2) and pairs.dtype == torch.int32 and m.shape == (9,) and m.dtype == torch.int32
    pairs, m = pairs.cpu().numpy(), m.cpu().numpy()
    for p, po in enumerate(batch["oracle"]):
        assert m[p] == len(po), f"pair {p}"
        np.testing.assert_array_equal(pairs[p, :m[p]], po, err_msg=f"pair {p}")
        assert (pairs[p, m[p]:] == -1).all(), f"pair {p}: tail"
    assert m[0] > 0 and m[8] > 0 and m[1] == 0 and m[2] == 0


@pytest.mark.parametrize("variant", ["314", "114"])
def test_match_ratio_equals_the_two_calls(variant, batch, monkeypatch):
    monkeypatch.setenv("MM_BF_VARIANT", variant)
    idx, dist = ops.bf_knn2_batched(batch["q"], batch["t"], batch["nq"], batch["nt"])
    pairs_o, m_o = ops.ratio_filter_batched(idx, dist, THRESHOLD, batch["nq"])
    pairs, m = ops.bf_match_ratio_batched(batch["q"], batch["t"], batch["nq"], batch["nt"], THRESHOLD)
    assert torch.equal(m, m_o)
    assert torch.equal(pairs, pairs_o)


def test_match_ratio_without_counts_and_single_pair():
    """nq = nt = NULL (every row valid) and the one-pair form (set strides 0)."""
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, (2, 130, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (2, 130, 32), dtype=np.uint8)
    q[:, :60] = t[:, 60:120]                # exact matches
    for n_pairs in (2, 1):
        qd, td = dev(q[:n_pairs]), dev(t[:n_pairs])
        pairs, m = ops.bf_match_ratio_batched(qd, td)
        idx, dist = ops.bf_knn2_batched(qd, td)
        pairs_o, m_o = ops.ratio_filter_batched(idx, dist, THRESHOLD)
        assert torch.equal(m, m_o) and torch.equal(pairs, pairs_o)
        assert int(m.min()) >= 60
        np.testing.assert_array_equal(pairs[0, :60].cpu().numpy(), np.stack([np.arange(60), np.arange(60) + 60], 1))


@pytest.mark.parametrize("variant", ["314"])
def test_rows_past_the_train_count_never_win(variant, monkeypatch):
    """The kernel stages its train tiles from the packed descriptors: rows in [nt, nt_cap) hold garbage (0xFF here) and
    rows in [nt_cap, next multiple of 32) do not exist (they read as 0 bits).  An all-ones and an all-zeros query would
    find them at distance 0.  nt = 290: inside the partial last tile; 288: the last tile is not touched; 300 = nt_cap."""
    monkeypatch.setenv("MM_BF_VARIANT", variant)
    rng = np.random.default_rng(17)
    nt = np.array([290, 288, 300], np.int32)
    q = rng.integers(0, 256, (3, CAP, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (3, CAP, 32), dtype=np.uint8)
    q[:, 0], q[:, 1] = 0xFF, 0x00
    for p in range(3):
        t[p, nt[p]:] = 0xFF
        t[p, 7] = flipped(np.full(32, 0xFF, np.uint8), [1, 2, 3])      # the true best of the all-ones query, d = 3
        t[p, 8] = flipped(np.zeros(32, np.uint8), [4, 5])              # ... and of the all-zeros query, d = 2
    pairs, m = ops.bf_match_ratio_batched(dev(q), dev(t), None, dev(nt), THRESHOLD)
    idx, dist = ops.bf_knn2_batched(dev(q), dev(t), None, dev(nt))
    pairs, m, idx, dist = pairs.cpu().numpy(), m.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()
    for p in range(3):
        io, do = oo.bf_knn2(q[p], t[p, :nt[p]])
        np.testing.assert_array_equal(idx[p], io)
        np.testing.assert_array_equal(dist[p], do)
        po = oo.ratio_filter(io, do, THRESHOLD)
        assert m[p] == len(po)
        np.testing.assert_array_equal(pairs[p, :m[p]], po)
        assert (pairs[p, m[p]:] == -1).all()
        assert list(pairs[p, 0]) == [0, 7] and list(pairs[p, 1]) == [1, 8]


# ---- what the plan (bf_plan in csrc/bf_match.hip) decides: kernel, splits, workspace ------------------------------------------

def planted(nq, nt, seed):
    """One pair of random rows with three planted queries; rows `hi` = nt - 1 and `hi` - k lie in the last 32-row tile.
      query 3: best row hi (d = 10), second row 1 (d = 40)          -> a match, the two in the last and the first split
      query 5: best row hi - 3 (d = 12), second row hi - 1 (d = 40) -> a match, both in the last tile
      query 7: row 2 and its copy at hi - 2, both d = 4             -> ties go to the lower index; never a match
      query 9: row hi - 6 and its copy at hi - 5, both d = 6        -> the same with both copies in the last tile
    Only the plants the train count has room for are made (nt >= 12); the oracle is the reference either way."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (1, nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (1, nt, 32), dtype=np.uint8)
    want = {}
    if nt >= 12 and nq > 9:
        hi, bits = nt - 1, rng.permutation(256)
        q[0, 3] = flipped(t[0, hi], bits[:10])
        t[0, 1] = flipped(t[0, hi], bits[10:40])
        q[0, 5] = flipped(t[0, hi - 3], bits[:12])
        t[0, hi - 1] = flipped(t[0, hi - 3], bits[12:40])
        t[0, hi - 2] = t[0, 2]
        q[0, 7] = flipped(t[0, 2], bits[:4])
        t[0, hi - 5] = t[0, hi - 6]
        q[0, 9] = flipped(t[0, hi - 6], bits[:6])
        want = {3: ([hi, 1], [10, 40]), 5: ([hi - 3, hi - 1], [12, 40]), 7: ([2, hi - 2], [4, 4]),
                9: ([hi - 6, hi - 5], [6, 6])}
    return q, t, want


def check_pair_against_oracle(q, t, want):
    """bf_knn2_batched exactly against the C oracle, bf_match_ratio_batched against the oracle's ratio filter and byte for
    byte against the two calls."""
    io, do = oo.bf_knn2(q[0], t[0])
    for qi, (ii, dd) in want.items():                # the plants are what they were meant to be
        assert list(io[qi]) == ii and list(do[qi]) == dd, (qi, io[qi], do[qi])
    qd, td = dev(q), dev(t)
    idx, dist = ops.bf_knn2_batched(qd, td)
    np.testing.assert_array_equal(idx[0].cpu().numpy(), io)
    np.testing.assert_array_equal(dist[0].cpu().numpy(), do)
    pairs_o, m_o = ops.ratio_filter_batched(idx, dist, THRESHOLD)
    pairs, m = ops.bf_match_ratio_batched(qd, td, None, None, THRESHOLD)
    assert torch.equal(m, m_o) and torch.equal(pairs, pairs_o)
    po = oo.ratio_filter(io, do, THRESHOLD)
    assert int(m[0]) == len(po)
    np.testing.assert_array_equal(pairs[0, :len(po)].cpu().numpy(), po)
    if want:
        assert [3, want[3][0][0]] in po.tolist() and [5, want[5][0][0]] in po.tolist()
        assert 7 not in po[:, 0] and 9 not in po[:, 0]


@pytest.mark.parametrize("nt_cap", [63, 64, 65535, 65536])
def test_dispatch_boundaries_without_the_environment(nt_cap, monkeypatch):
    """The matrix-core kernel takes 64 <= nt_cap < 65536, the popcount kernel the rest (the layouts on either side:
    test_match_stage_abi.py).  70 queries; the plants sit in the last 32-row tile, which is partial at 63 and 65535; at
    65536 the best of query 3 is row 65535, the last index the matrix-core kernel's 16-bit train indices could hold."""
    monkeypatch.delenv("MM_BF_VARIANT", raising=False)
    q, t, want = planted(70, nt_cap, seed=nt_cap)
    assert want[3][0][0] == nt_cap - 1
    check_pair_against_oracle(q, t, want)


@pytest.mark.parametrize("variant", ["114", None])
@pytest.mark.parametrize("nt", [1, 2, 63])
def test_single_query_single_split(nt, variant, monkeypatch):
    """nq = 1 at nt_cap = 63 (one split, whatever the environment says): one, two and 63 valid trains."""
    if variant is None:
        monkeypatch.delenv("MM_BF_VARIANT", raising=False)
    else:
        monkeypatch.setenv("MM_BF_VARIANT", variant)
    from meatmodeler_amd import _lib
    assert _lib.lib.mm_bf_workspace_bytes(1, 1, 63) == 256          # one split: no partial keys
    rng = np.random.default_rng(nt)
    q = rng.integers(0, 256, (1, 1, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (1, 63, 32), dtype=np.uint8)
    t[0, nt:] = q[0, 0]                                             # rows past the count would win at distance 0
    t[0, nt - 1] = flipped(q[0, 0], [9, 99])                        # the true best: the last valid row, d = 2
    io, do = oo.bf_knn2(q[0], t[0, :nt])
    assert io[0, 0] == nt - 1 and do[0, 0] == 2 and (io[0, 1] == -1) == (nt == 1)
    ntd = dev(np.array([nt], np.int32))
    idx, dist = ops.bf_knn2_batched(dev(q), dev(t), None, ntd)
    np.testing.assert_array_equal(idx[0].cpu().numpy(), io)
    np.testing.assert_array_equal(dist[0].cpu().numpy(), do)
    pairs, m = ops.bf_match_ratio_batched(dev(q), dev(t), None, ntd, THRESHOLD)
    po = oo.ratio_filter(io, do, THRESHOLD)
    assert int(m[0]) == len(po) == (0 if nt == 1 else 1)
    np.testing.assert_array_equal(pairs[0, :len(po)].cpu().numpy(), po)
    assert (pairs[0, len(po):] == -1).all()


@pytest.mark.parametrize("nt,splits", [(127, 1), (128, 1), (129, 2), (257, 3)])
def test_split_and_merge_at_the_split_rule(nt, splits, monkeypatch):
    """The popcount kernel on one small pair splits its train range, at least 128 trains per split: 1, 1, 2, 3 splits.
    Query 3 has its best in the last split and its second best in the first, query 7 a tie across them."""
    monkeypatch.setenv("MM_BF_VARIANT", "114")
    from meatmodeler_amd import _lib
    knn = _lib.lib.mm_bf_workspace_bytes(1, 70, nt)
    assert knn == (256 if splits == 1 else (splits * 70 * 2 * 4 + 255) // 256 * 256)      # partial keys of every split
    q, t, want = planted(70, nt, seed=nt)
    check_pair_against_oracle(q, t, want)


def test_removed_variants_are_refused(monkeypatch):
    from meatmodeler_amd._lib import MMError
    q, t, _ = planted(10, 70, seed=1)
    monkeypatch.setenv("MM_BF_VARIANT", "300")
    with pytest.raises(MMError, match=r"\(-1\)") as err:            # MM_ERR_ARG
        ops.bf_knn2_batched(dev(q), dev(t))
    assert "314" in str(err.value) and "114" in str(err.value) and "removed" in str(err.value)
    with pytest.raises(MMError, match=r"\(-1\)"):
        ops.bf_match_ratio_batched(dev(q), dev(t))
    monkeypatch.delenv("MM_BF_VARIANT")
    idx, dist = ops.bf_knn2_batched(dev(q), dev(t))
    io, do = oo.bf_knn2(q[0], t[0])
    np.testing.assert_array_equal(idx[0].cpu().numpy(), io)
    np.testing.assert_array_equal(dist[0].cpu().numpy(), do)
