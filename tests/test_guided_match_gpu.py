"""GPU: mm_guided_match through ops.guided_match, processor.guidedMatching and ClipPipeline.run(guided=...) against the NumPy
restatement of tests/test_guided_match_cpu.py.

Shapes: n_pairs <= 4, cap = 320.  Every output is an integer and every comparison is equality: pairs_out with its -1 tail,
m_out, is_new, info.  The fixtures keep every (query, train) combination more than 1e-6 relative from tau^2 (asserted in the
CPU file), so a gate disagreement is a bug, not rounding.  The boundaries vary one thing at a time: n_q and n_t independently
in {0, 1, 2, 63, 64, 65, 255, 256, 257, 320} (the search works on tiles of 256 queries x 256 trains, the lists on rounds of 256:
255 / 256 / 257 are the tile edges), m in {0, 1, n_q}, threshold_px in {0, inf}, max_dist in {0, 256}, ratio in {0, 1}.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_guided_match_cpu as ref  # noqa: E402
from meatmodeler_amd import _lib, ops, processor, synth  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402

DEV = torch.device("cuda", 0)
CAP = ref.CAP
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 320)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def run(kp, desc, n, pairs, m, model, kind=None, **kw):
    """-> (pairs_out, m_out, is_new, info) as NumPy arrays."""
    kd = None if kind is None else dev(np.asarray(kind, np.int32))
    return tuple(t.cpu().numpy() for t in ops.guided_match(dev(kp), dev(desc), dev(np.asarray(n, np.int32)), dev(pairs),
                                                           dev(np.asarray(m, np.int32)), dev(np.asarray(model, np.float64)),
                                                           kind=kd, **kw))


def check(got, want, what=""):
    for g, w, name in zip(got, want, ("pairs_out", "m_out", "is_new", "info")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())


def both(args, kind=None, what="", **kw):
    """One call on the GPU against the restatement; returns the GPU's arrays."""
    prm = dict(ref.DEFAULTS)
    prm.update(kw)
    got = run(*args, kind=kind, **dict(prm, cross_check=bool(prm["cross_check"])))
    check(got, ref.guided_numpy(*args, kind=kind, **prm), what)
    return got


def rows_of(seeds, cap=CAP):
    out = np.full((cap, 2), -1, np.int32)
    out[:len(seeds)] = seeds
    return out


def one_pair(t, seeds, n_q=None, n_t=None):
    """The arguments of a one-pair call on the tables t."""
    n = np.array([t["n"][0] if n_q is None else n_q, t["n"][1] if n_t is None else n_t], np.int32)
    return (t["kp"], t["desc"], n, rows_of(seeds)[None], np.array([len(seeds)], np.int32), np.asarray(t["model"]).reshape(1, 9))


def four_pairs(t, which="A"):
    """Frames Q, T, Q, T, Q of one scene: pairs 0 and 2 in the scene's direction, 1 and 3 in the other (F^T / adj H)."""
    back = ref.reversed_tables(t)
    s = ref.seeds_of(t, which)
    sb = ref.reversed_seeds(s)
    kp = np.stack([t["kp"][0], t["kp"][1], t["kp"][0], t["kp"][1], t["kp"][0]])
    desc = np.stack([t["desc"][0], t["desc"][1], t["desc"][0], t["desc"][1], t["desc"][0]])
    n = np.array([t["n"][0], t["n"][1], t["n"][0], t["n"][1], t["n"][0]], np.int32)
    pairs = np.stack([rows_of(s), rows_of(sb), rows_of(s), rows_of(sb)])
    m = np.array([len(s), len(sb), len(s), len(sb)], np.int32)
    model = np.stack([t["model"], back["model"], t["model"], back["model"]])
    return [kp, desc, n, pairs, m, model], np.full(4, t["kind"], np.int32)


@pytest.mark.parametrize("seed,planar", ref.GPU_SEEDS)
def test_fixtures_in_both_directions(seed, planar):
    t = ref.tables(seed, planar)
    kind = [t["kind"]]
    for tt in (t, ref.reversed_tables(t)):
        for cc in (0, 1):
            r = both(one_pair(tt, ref.seeds_of(tt, "A")), kind, f"A cc={cc}", cross_check=cc)
            # the decoyed points come back (which ones: the CPU file); seen from the train image the ratio test loses nothing
            assert r[3][0, 2] >= 58 if tt is t else r[3][0, 2] == 0
            for ratio, max_dist in ((0.8, 64), (1.0, 256)):
                for tau in (40.0, ref.DENSE_TAU[planar]):
                    both(one_pair(tt, ref.seeds_of(tt, "B")), kind, f"B tau={tau} cc={cc} ratio={ratio}", threshold_px=tau,
                         ratio=ratio, max_dist=max_dist, cross_check=cc)


def test_default_kind_is_a_fundamental_matrix():
    t = ref.tables(0)
    args = one_pair(t, ref.seeds_of(t, "A"))
    check(run(*args), ref.guided_numpy(*args, kind=[0], **ref.DEFAULTS), "kind=None")


def test_four_pairs_no_model_nan_unordered_malformed():
    args, kind = four_pairs(ref.tables(0))
    kp, desc, n, pairs, m, model = args
    kind = kind.copy()
    kind[0] = -1                                   # pair 0: no model
    model = model.copy()
    model[1, 7] = math.nan                         # pair 1: a NaN in its model
    pairs = pairs.copy()
    pairs[2, [10, 11]] = pairs[2, [11, 10]]        # pair 2: seeds out of order
    pairs[3, 20, 1] = CAP                          # pair 3: a train index outside the table
    for cc in (0, 1):
        got = both((kp, desc, n, pairs, m, model), kind, f"cc={cc}", cross_check=cc)
        assert got[3][:, 0].tolist() == [ref.SKIPPED, ref.SKIPPED, ref.UNORDERED, ref.MALFORMED]
        assert np.array_equal(got[0][:3], pairs[:3]) and np.array_equal(got[1][:3], m[:3]) and not got[2][:3].any()
        assert got[3][3, 1] == m[3] - 1 and got[3][3, 2] > 0
    pairs[2, 5, 0] = -7                            # a malformed row in a pair that passes through: copied, and flagged
    got = both((kp, desc, n, pairs, m, model), kind)
    assert got[3][2, 0] == ref.UNORDERED | ref.MALFORMED and np.array_equal(got[0][2], pairs[2])


@pytest.mark.parametrize("planar", [False, True])
def test_key_point_counts_at_every_boundary(planar):
    t = ref.tables(0, planar)
    seeds = ref.seeds_of(t, "B")
    full = dict(t, n=np.array([CAP, CAP], np.int32))      # rows beyond the tables' own counts are zero key points: still rows
    tau = ref.DENSE_TAU[planar]
    for n_q in SIZES:
        for n_t in SIZES:
            s = seeds[(seeds[:, 0] < n_q) & (seeds[:, 1] < n_t)]
            both(one_pair(full, s, n_q, n_t), [t["kind"]], f"n_q={n_q} n_t={n_t}", threshold_px=tau)
    # counts outside 0 .. cap are clamped; seeds beyond the counts are kept and mark rows nobody searches
    both(one_pair(full, seeds, -3, CAP + 50), [t["kind"]], "clamped", threshold_px=tau)
    both(one_pair(full, seeds, 100, 90), [t["kind"]], "seeds beyond n", threshold_px=tau)


def test_seed_counts():
    t = ref.tables(1)
    seeds = ref.seeds_of(t, "B")
    n_q = int(t["n"][0])
    for m in (0, 1):
        both(one_pair(t, seeds[:m]), [0], f"m={m}", threshold_px=40.0)
    every = np.stack([np.arange(n_q), np.arange(n_q)], axis=1).astype(np.int32)      # all queries used: nothing is added
    got = both(one_pair(t, every), [0], "m=n_q", threshold_px=math.inf, ratio=1.0, max_dist=256)
    assert got[3][0].tolist() == [0, n_q, 0, 0] and np.array_equal(got[0][0, :n_q], every)
    # m beyond cap is clamped, a negative m is none
    args = list(one_pair(t, seeds))
    for m in (-4, CAP + 9):
        args[4] = np.array([m], np.int32)
        args[3] = rows_of(np.stack([np.arange(CAP), np.arange(CAP)], axis=1))[None]
        both(tuple(args), [0], f"m={m}", threshold_px=40.0)


@pytest.mark.parametrize("planar", [False, True])
def test_parameter_extremes(planar):
    t = ref.tables(0, planar)
    seeds = ref.seeds_of(t, "B")
    base = dict(threshold_px=ref.DENSE_TAU[planar], ratio=0.8, max_dist=64)
    for change in (dict(threshold_px=0.0), dict(threshold_px=math.inf), dict(max_dist=0), dict(max_dist=256), dict(ratio=0.0),
                   dict(ratio=1.0), dict(threshold_px=math.inf, ratio=1.0, max_dist=256)):
        for cc in (0, 1):
            both(one_pair(t, seeds), [t["kind"]], str(change), **dict(base, cross_check=cc, **change))


def test_without_gate_and_seeds_it_is_the_match_stage():
    """tau = inf, no seeds, cross_check = 0, max_dist = 256 against the existing kernel: bf_match_ratio_batched's matches on the
    same tables, resolved to the lowest (distance, query) per train."""
    t = ref.tables(0)
    nq, nt = int(t["n"][0]), int(t["n"][1])
    for ratio in (0.75, 1.0):
        pairs, m = ops.bf_match_ratio_batched(dev(t["desc"][0:1]), dev(t["desc"][1:2]), dev(t["n"][0:1]), dev(t["n"][1:2]), ratio)
        rows = pairs[0, :int(m[0].item())].cpu().numpy()
        D = ref.hamming_all(t["desc"][0, :nq], t["desc"][1, :nt])
        want = ref.lowest_per_train([(q, j, D[q, j]) for q, j in rows.tolist()])
        got = both(one_pair(t, np.zeros((0, 2), np.int32)), [0], f"ratio={ratio}", threshold_px=math.inf, ratio=ratio, max_dist=256,
                   cross_check=0)
        assert got[1][0] == len(want) and np.array_equal(got[0][0, :len(want)], want) and got[2][0, :len(want)].all()


def test_invariances():
    args, kind = four_pairs(ref.tables(1), "B")
    kp, desc, n, pairs, m, model = args
    kind = kind.copy()
    kw = dict(threshold_px=40.0, ratio=1.0, max_dist=256)
    whole = both(tuple(args), kind, "whole", **kw)
    again = run(*args, kind=kind, **kw)
    check(again, whole, "repeated")
    for p in range(4):
        alone = run(kp[p:p + 2], desc[p:p + 2], n[p:p + 2], pairs[p:p + 1], m[p:p + 1], model[p:p + 1], kind=kind[p:p + 1], **kw)
        check(alone, tuple(a[p:p + 1] for a in whole), f"pair {p} alone")
    block = run(kp[1:4], desc[1:4], n[1:4], pairs[1:3], m[1:3], model[1:3], kind=kind[1:3], **kw)
    check(block, tuple(a[1:3] for a in whole), "rows [1, 3)")
    # what shares the call does not matter either: the same pair beside a skipped one
    kind2 = kind.copy()
    kind2[0] = 5
    other = run(*args, kind=kind2, **kw)
    check(tuple(a[1:] for a in other), tuple(a[1:] for a in whole), "neighbour skipped")


def test_argument_and_workspace_errors():
    t = ref.tables(0)
    args = [dev(a) for a in one_pair(t, ref.seeds_of(t, "A"))]
    for bad in (dict(threshold_px=-1.0), dict(threshold_px=math.nan), dict(ratio=-1.0), dict(ratio=math.nan), dict(max_dist=-1),
                dict(max_dist=257)):
        with pytest.raises(ValueError):
            ops.guided_match(*args, **bad)
    with pytest.raises(ValueError):
        ops.guided_match(args[0], args[1][:, :100], *args[2:])
    with pytest.raises(ValueError):
        ops.guided_match(*args, kind=dev(np.zeros(2, np.int32)))
    # through the library with a live context: the checks come first
    ctx = _lib.default_context()
    import ctypes as C
    need = _lib.lib.mm_guided_workspace_bytes(1, CAP)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = [torch.empty((1, CAP, 2), dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV),
           torch.empty((1, CAP), dtype=torch.uint8, device=DEV), torch.empty((1, 4), dtype=torch.int32, device=DEV)]

    def call(prm, ws_bytes=need, pairs_out=out[0]):
        return _lib.lib.mm_guided_match(ctx.h, *[_lib.ptr(a) for a in args], None, 1, CAP, C.byref(prm), _lib.ptr(pairs_out),
                                        *[_lib.ptr(o) for o in out[1:]], _lib.ptr(ws), ws_bytes)

    good = _lib.GuidedParams(2.0, 0.8, 64, 1)
    assert call(good) == 0
    assert call(good, ws_bytes=need - 1) == -3 and b"workspace" in _lib.lib.mm_last_error(ctx.h)
    assert call(_lib.GuidedParams(2.0, 0.8, 64, 2)) == -1 and call(_lib.GuidedParams(2.0, 0.8, 300, 1)) == -1
    assert call(good, pairs_out=args[3]) == -1
    ctx.sync()
    # no pairs: nothing is launched, empty outputs
    e = ops.guided_match(args[0][:1], args[1][:1], args[2][:1], args[3][:0], args[4][:0], args[5][:0])
    assert [tuple(x.shape) for x in e] == [(0, CAP, 2), (0,), (0, CAP), (0, 4)]


def test_processor_wrapper():
    t = ref.tables(0)
    nq, nt = int(t["n"][0]), int(t["n"][1])
    seeds = ref.seeds_of(t, "A")
    rows, new = processor.guidedMatching(t["kp"][0, :nq], t["desc"][0, :nq], t["kp"][1, :nt], t["desc"][1, :nt], seeds,
                                         np.asarray(t["model"]).reshape(3, 3))
    want = ref.run_fixture(t, "A")
    assert np.array_equal(rows, want["rows"]) and np.array_equal(new, want["is_new"].astype(bool))
    p = ref.tables(0, True)
    rows, new = processor.guidedMatching(p["kp"][0, :nq], p["desc"][0, :nq], p["kp"][1, :nt], p["desc"][1, :nt], ref.seeds_of(p, "A"),
                                         np.asarray(p["model"]).reshape(3, 3), homography=True, cross_check=False)
    want = ref.run_fixture(p, "A", cross_check=0)
    assert np.array_equal(rows, want["rows"]) and np.array_equal(new, want["is_new"].astype(bool))


@functools.lru_cache(maxsize=None)
def clip():
    frames, ext, K = synth.render_orbit_frames(6, 640, 480, arc_deg=6.0)
    return dev(frames), ext, K


def test_run_with_guided():
    frames, ext, K = clip()
    pipe = ClipPipeline(480, 640, 600, batch=6)
    keys = ("track_ptr_dev", "obs_frame_dev", "obs_kp_dev", "points0")
    # guided=None launches what it launched before: the same tensors as the run without the argument, verified or not
    plain, none = pipe.run(frames, K, ext, ba=False), pipe.run(frames, K, ext, ba=False, guided=None)
    verified, verified_none = pipe.run(frames, K, ext, ba=False, verify={}), pipe.run(frames, K, ext, ba=False, verify={}, guided=None)
    for a, b in ((plain, none), (verified, verified_none)):
        assert "guided" not in b
        for k in keys:
            assert torch.equal(a[k], b[k])
        assert np.array_equal(a["match_count"], b["match_count"])
    for k in ("info", "cost", "F"):
        assert torch.equal(verified["verify"][k], verified_none["verify"][k])
    with pytest.raises(ValueError, match="guided needs verify"):
        pipe.run(frames, K, ext, ba=False, guided={})
    with pytest.raises(ValueError):
        pipe.run(frames, K, ext, ba=False, verify={}, guided=dict(tau=2.0))
    timers = {}
    out = pipe.run(frames, K, ext, ba=False, verify={}, guided={}, timers=timers)
    assert timers["guided"] > 0.0 and "guided" not in pipe.run(frames, K, ext, ba=False, verify={}, timers={})
    g = out["guided"]
    assert g["info"].shape == (5, 4) and g["info"].dtype == torch.int32 and g["is_new"].shape == (5, 600)
    added = int(g["info"][:, 2].sum().item())
    print(f"observations {verified['n_obs']} -> {out['n_obs']}, tracks {verified['n_tracks']} -> {out['n_tracks']}, {added} matches added")
    assert out["n_obs"] >= verified["n_obs"] and added >= 0
    assert np.array_equal(out["match_count"], verified["match_count"] + g["info"][:, 2].cpu().numpy())
    # its entries are those of a direct call on the same inputs
    det = out["det"]
    pairs_in, m_in = pipe.match(det)
    pairs_v, m_v, F_v, _, info_v = pipe.verify(det, pairs_in, m_in)
    assert torch.equal(info_v, out["verify"]["info"])
    kind = torch.where((info_v[:, 0] & 7) != 0, -1, 0).to(torch.int32)
    po, mo, new, info = ops.guided_match(det["xy"], det["desc"], det["n"], pairs_v, m_v, F_v, kind=kind)
    assert torch.equal(info, g["info"]) and torch.equal(new, g["is_new"])
    assert np.array_equal(mo.cpu().numpy(), out["match_count"])
    # with degeneracy the homography is the model where the verdict says so
    deg = pipe.run(frames, K, ext, ba=False, verify={}, degeneracy={}, guided={})
    assert deg["guided"]["info"].shape == (5, 4) and deg["n_obs"] >= pipe.run(frames, K, ext, ba=False, verify={}, degeneracy={})["n_obs"]
