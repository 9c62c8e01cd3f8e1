"""GPU: the index build of a BA problem (mm_ba_index_build, what ops.BADevice holds) against the NumPy statement of the
same structures (oracle.ba_oracle.index_reference, itself checked against the host builders in tests/test_host_logic.py),
array by array.  Everything is integer data: equality is exact.

Run on the MI355X box:  python -m pytest tests/test_ba_index_gpu.py -m gpu -q
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from meatmodeler_amd import ops, synth  # noqa: E402
from oracle import ba_oracle as bo  # noqa: E402

DEV = torch.device("cuda", 0)
K = synth.default_K(1920, 1080)
CSR = ("pt_ptr", "pt_obs", "cam_ptr", "cam_obs")
PAIRS = ("pair_o", "pair_o2", "pair_p", "seg_ids", "seg_chunk_ptr", "chunk_seg", "chunk_begin", "chunk_end")


def build(fi, pi, F, P, **kw):
    fi, pi = np.asarray(fi, np.int32), np.asarray(pi, np.int32)
    return ops.BADevice(K, fi, pi, np.zeros((fi.size, 2)), F, P, DEV, **kw)


def fixed(n):
    return torch.zeros((n, 6), dtype=torch.float64, device=DEV)


def same_index(fi, pi, F, P, want_pairs=True, **kw):
    """The build of one problem and its reference, compared attribute by attribute.  -> the BADevice."""
    a = build(fi, pi, F, P, **kw)
    F_fixed = 0 if kw.get("fixed_cams") is None else int(kw["fixed_cams"].shape[0])
    b = bo.index_reference(fi, pi, F, P, F_fixed, ops.BADevice._chunk_pairs(), kw.get("max_band_span", 192), kw.get("pairs", True))
    assert a.F_fixed == F_fixed
    for name in CSR:
        x, y = getattr(a, name), b[name]
        assert x.dtype == torch.int32 and y.dtype == np.int32 and x.is_contiguous()
        np.testing.assert_array_equal(x.cpu().numpy(), y, err_msg=name)
    assert a.cam_span == b["cam_span"] and a.n_pairs == b["n_pairs"]
    assert (a.pb.cam_span, a.pb.n_seg, a.pb.n_chunks) == (b["cam_span"], len(b.get("seg_ids", ())), len(b.get("chunk_seg", ())))
    assert (a.n_pairs > 0) == want_pairs
    for name in PAIRS:
        assert hasattr(a, name) == (name in b) == want_pairs, name
        if want_pairs:
            x, y = getattr(a, name), b[name]
            assert x.dtype == torch.int32 and y.dtype == np.int32 and x.is_contiguous()
            np.testing.assert_array_equal(x.cpu().numpy(), y, err_msg=name)
    sa, sb = a.slabs, b["slabs"]
    assert (sa is None) == (sb is None)
    if sa is not None:
        assert sa[:2] == sb[:2]
        np.testing.assert_array_equal(sa[2], sb[2])
        np.testing.assert_array_equal(sa[3], sb[3])
    return a


def two_cameras(n_shared):
    """2 cameras x n_shared points seen by both: segments (0, 0), (1, 0) and (1, 1) of n_shared pairs each."""
    pi = np.repeat(np.arange(n_shared), 2)
    fi = np.tile(np.array([0, 1]), n_shared)
    return fi, pi


def test_empty_and_single_observation():
    e = same_index(np.zeros(0), np.zeros(0), 3, 2, want_pairs=False)
    assert e.n_pairs == 0 and e.cam_span == 0
    # one point with one observation (camera 1 of 3, point 1 of 3: empty bins on both sides)
    pb = same_index([1], [1], 3, 3)
    assert pb.n_pairs == 1 and pb.pb.n_seg == 1 and pb.pb.n_chunks == 1 and pb.cam_span == 0


def test_every_point_observed_once_has_only_diagonal_pairs():
    rng = np.random.default_rng(0)
    P, F = 700, 9
    fi = rng.integers(0, F - 1, P)                          # (camera 8 observes nothing)
    pb = same_index(fi, np.arange(P), F, P)
    assert pb.n_pairs == P and pb.cam_span == 0
    np.testing.assert_array_equal(pb.pair_o.cpu().numpy(), pb.pair_o2.cpu().numpy())


@pytest.mark.parametrize("chunk,cuts", [("64", [64] * 9 + [24]), ("512", [512, 88])])
def test_segments_of_600_pairs_cut_into_chunks(chunk, cuts, monkeypatch):
    monkeypatch.setenv("MM_SCHUR_CHUNK", chunk)
    fi, pi = two_cameras(600)
    pb = same_index(fi, pi, 2, 600)
    assert pb.n_pairs == 1800 and pb.pb.n_seg == 3 and pb.pb.n_chunks == 3 * len(cuts)
    sizes = (pb.chunk_end - pb.chunk_begin).cpu().numpy()
    assert list(sizes) == cuts * 3


@pytest.mark.parametrize("n_shared", [63, 64, 65])
def test_segments_at_the_chunk_size(n_shared, monkeypatch):
    monkeypatch.setenv("MM_SCHUR_CHUNK", "64")
    fi, pi = two_cameras(n_shared)
    pb = same_index(fi, pi, 2, n_shared)
    assert pb.pb.n_chunks == (3 if n_shared <= 64 else 6)


@pytest.mark.parametrize("seed", [3, 4])
def test_mixed_track_lengths(seed):
    """12 cameras x 300 points, tracks of 1 .. 6 observations from random (not consecutive) cameras, two points nobody
    observes and one observed twice by the same camera."""
    rng = np.random.default_rng(seed)
    F, P = 12, 300
    fi, pi = [], []
    for p in range(P):
        if p in (17, 299):
            continue
        cams = np.sort(rng.choice(F, rng.integers(1, 7), replace=False))
        if p == 40:
            cams = np.sort(np.append(cams, cams[0]))
        fi += list(cams)
        pi += [p] * len(cams)
    pb = same_index(fi, pi, F, P)
    assert pb.n_pairs > len(fi)
    pr = synth.make_ba_problem(12, 300, 4, seed=seed)
    same_index(pr["fi"], pr["pi"], 12, 300)


def test_camera_slabs_from_the_native_arrays():
    """130 cameras: 8 slabs of 17 cameras, computed on first use from the arrays the build returned."""
    pr = synth.make_ba_problem(130, 400, 5, seed=2)
    pb = same_index(pr["fi"], pr["pi"], 130, 400)
    assert pb.slabs is not None and pb.slabs[:2] == (8, 17)


def test_band_edges():
    # cam_span == F - 1, the widest there is: the band condition (cam_span < F) still holds, the list spans every block
    fi, pi = [0, 3, 1, 2], [0, 0, 1, 1]
    pb = same_index(fi, pi, 4, 2)
    assert pb.cam_span == 3 and pb.n_pairs == 6
    # cam_span == max_band_span: pair list; max_band_span + 1: none
    fi, pi = [0, 5, 2, 3, 9], [0, 0, 1, 1, 2]
    assert same_index(fi, pi, 10, 3, max_band_span=5).cam_span == 5
    assert same_index(fi, pi, 10, 3, max_band_span=4, want_pairs=False).cam_span == 5
    # pairs=False: CSRs and span only
    assert same_index(fi, pi, 10, 3, pairs=False, want_pairs=False).cam_span == 5


def problem_12x300():
    pr = synth.make_ba_problem(12, 300, 4, seed=5)
    fi, pi = pr["fi"].astype(np.int32), pr["pi"].astype(np.int32)
    return fi, pi, np.random.default_rng(1).permutation(fi.size)


def test_fixed_cameras_and_other_orders_are_built_natively():
    fi, pi, perm = problem_12x300()
    # not point-major: stage 0 reports it and runs again with the sort by point
    pb = same_index(fi[perm], pi[perm], 12, 300)
    assert pb.n_pairs > 0 and not pb.point_major
    # fixed cameras (cameras 10, 11 observed but not optimised): 10 free + 2 fixed cameras x 300 points
    a = same_index(fi, pi, 10, 300, fixed_cams=fixed(2))
    assert a.F_fixed == 2 and a.point_major and 0 < a.cam_obs.numel() < fi.size
    # both at once
    b = same_index(fi[perm], pi[perm], 10, 300, fixed_cams=fixed(2))
    assert b.n_pairs == a.n_pairs and b.cam_span == a.cam_span


def test_points_and_cameras_that_fixed_cameras_leave_empty():
    # point 1 is seen by fixed cameras only (3 free + 2 fixed cameras): it has observations, but no pairs
    fi, pi = [0, 1, 3, 4, 2, 3, 0], [0, 0, 1, 1, 2, 2, 3]
    pb = same_index(fi, pi, 3, 4, fixed_cams=fixed(2))
    assert pb.n_pairs == 5 and 1 not in pb.pair_p.cpu().numpy() and pb.cam_obs.numel() == 4
    # every observation is of a fixed camera: CSR by point only, no pair list, no span
    pb = same_index([2, 3, 2], [0, 0, 1], 2, 2, want_pairs=False, fixed_cams=fixed(2))
    assert pb.cam_span == 0 and pb.cam_obs.numel() == 0 and pb.cam_ptr.cpu().tolist() == [0, 0, 0]
    pb = same_index([0, 1, 0], [0, 0, 1], 0, 2, want_pairs=False, fixed_cams=fixed(2))      # (no free camera at all)
    assert pb.cam_ptr.cpu().tolist() == [0]
    # the highest fixed index is observed and the last free camera (3 of 4 + 3) observes nothing: cam_ptr ends at its bins
    rng = np.random.default_rng(6)
    cams = np.array([0, 1, 2, 4, 5, 6])
    fi = np.concatenate([np.sort(rng.choice(cams, 3, replace=False)) for _ in range(100)])
    fi[-1] = 6
    pi = np.repeat(np.arange(100), 3)
    for order in (np.arange(300), rng.permutation(300)):
        pb = same_index(fi[order], pi[order], 4, 100, fixed_cams=fixed(3))
        ptr = pb.cam_ptr.cpu().numpy()
        assert ptr[3] == ptr[4] == pb.cam_obs.numel() and pb.n_pairs > 0


def test_permuted_observations_whose_first_and_last_points_are_unobserved():
    fi, pi, perm = problem_12x300()
    pb = same_index(fi[perm], pi[perm] + 1, 12, 302)
    ptr = pb.pt_ptr.cpu().numpy()
    assert ptr[0] == ptr[1] == 0 and ptr[-1] == ptr[-2] == fi.size


@pytest.mark.parametrize("order", ["point-major", "permuted"])
def test_an_index_out_of_range_is_refused(order):
    fi, pi, perm = problem_12x300()
    if order == "permuted":
        fi, pi = fi[perm], pi[perm]
    for F, kw in ((12, {}), (10, dict(fixed_cams=fixed(2)))):
        build(fi, pi, F, 300, **kw)
        for bad_f, bad_p in ((12, 0), (-1, 0), (0, 300), (0, -1)):      # (12 == F + F_fixed)
            f2, p2 = fi.copy(), pi.copy()
            f2[150], p2[150] = bad_f, bad_p
            with pytest.raises(ValueError, match="frame / point index out of range"):
                build(f2, p2, F, 300, **kw)
    with pytest.raises(ValueError):
        build([0, 12], [0, 1], 12, 300)
    with pytest.raises(ValueError):
        build([0, 1], [0, -1], 12, 300)
    with pytest.raises(ValueError):
        build([0], [0], 3, 0)


def solve_problems():
    """name -> (K, fi, pi, obs, F free cameras, cams0 [12, 6], pts0 [300, 3]): the 12 x 300 problem with its observations
    permuted, and with cameras 10 and 11 fixed at their initial values."""
    pr = synth.make_ba_problem(12, 300, 4, seed=7)
    cams0 = bo.frame_parameters(pr["ext"]).reshape(12, 6)
    fi, pi, obs = pr["fi"].astype(np.int32), pr["pi"].astype(np.int32), pr["obs"]
    perm = np.random.default_rng(2).permutation(fi.size)
    return dict(permuted=(pr["K"], fi[perm], pi[perm], obs[perm], 12, cams0, pr["pts0"]),
                fixed=(pr["K"], fi, pi, obs, 10, cams0, pr["pts0"]))


def solve(K, fi, pi, obs, F, cams0, pts0):
    """-> (BADevice, cams [F, 6], pts, cost, nfev) of one trf_solve from (cams0, pts0)."""
    c, p = torch.as_tensor(cams0[:F].copy()).to(DEV), torch.as_tensor(pts0.copy()).to(DEV)
    kw = dict(fixed_cams=torch.as_tensor(cams0[F:].copy()).to(DEV)) if F < len(cams0) else {}
    pb = ops.BADevice(K, fi, pi, obs, F, len(pts0), DEV, **kw)
    rep, _ = pb.trf_solve(c, p, 1e-6, 1e-8, 1e-8)
    return pb, c.cpu().numpy(), p.cpu().numpy(), float(rep.cost), int(rep.nfev)


@pytest.mark.parametrize("name", ["permuted", "fixed"])
def test_solver_is_bitwise_what_the_parent_build_gave(name, golden_dir):
    """The solve of a problem whose index structures commit 9b0cfbd still assembled from torch sorts and scans: cameras,
    points, cost and nfev equal, bit for bit, what that commit returned on an MI355X (tests/golden, saved there once)."""
    pb, cams, pts, cost, nfev = solve(*solve_problems()[name])
    assert pb.n_pairs > 0
    g = np.load(os.path.join(golden_dir, "ba_index_solve_parent_9b0cfbd.npz"))
    print(f"{name}: cost {cost!r} (golden {float(g[name + '_cost'])!r}), nfev {nfev} (golden {int(g[name + '_nfev'])})")
    assert cost == float(g[name + "_cost"]) and nfev == int(g[name + "_nfev"])
    assert torch.equal(torch.as_tensor(cams), torch.as_tensor(g[name + "_cams"]))
    assert torch.equal(torch.as_tensor(pts), torch.as_tensor(g[name + "_pts"]))
