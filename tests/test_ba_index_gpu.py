"""GPU: the native index build of a BA problem (mm_ba_index_build, what ops.BADevice uses for point-major problems without
fixed cameras) against the construction from torch sorts / scans it replaces (BADevice(..., native_index=False)), array
by array.  Everything is integer data: equality is exact.

Run on the MI355X box:  python -m pytest tests/test_ba_index_gpu.py -m gpu -q
"""
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


def build(fi, pi, F, P, native, **kw):
    fi, pi = np.asarray(fi, np.int32), np.asarray(pi, np.int32)
    return ops.BADevice(K, fi, pi, np.zeros((fi.size, 2)), F, P, DEV, native_index=native, **kw)


def same_index(fi, pi, F, P, want_pairs=True, want_build="native", **kw):
    """Both builds of one problem, compared attribute by attribute.  -> the native one."""
    a, b = build(fi, pi, F, P, True, **kw), build(fi, pi, F, P, False, **kw)
    assert a.index_build == want_build and b.index_build == "torch"
    for name in CSR:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype == torch.int32 and x.is_contiguous()
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=name)
    assert a.cam_span == b.cam_span and a.n_pairs == b.n_pairs
    assert (a.pb.cam_span, a.pb.n_seg, a.pb.n_chunks) == (b.pb.cam_span, b.pb.n_seg, b.pb.n_chunks)
    assert (a.n_pairs > 0) == want_pairs
    for name in PAIRS:
        assert hasattr(a, name) == hasattr(b, name) == want_pairs, name
        if want_pairs:
            x, y = getattr(a, name), getattr(b, name)
            assert x.dtype == y.dtype == torch.int32 and x.is_contiguous()
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=name)
    sa, sb = a.slabs, b.slabs
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
    e = build(np.zeros(0), np.zeros(0), 3, 2, True)
    t = build(np.zeros(0), np.zeros(0), 3, 2, False)
    for name in CSR:
        np.testing.assert_array_equal(getattr(e, name).cpu().numpy(), getattr(t, name).cpu().numpy())
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
    """130 cameras: 8 slabs of 17 cameras, computed on first use from the arrays the native build returned."""
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


def test_fixed_cameras_and_other_orders_keep_the_torch_build():
    pr = synth.make_ba_problem(12, 300, 4, seed=5)
    fi, pi = pr["fi"].astype(np.int32), pr["pi"].astype(np.int32)
    # not point-major: the native build declines, the result is the torch build's
    perm = np.random.default_rng(1).permutation(fi.size)
    pb = same_index(fi[perm], pi[perm], 12, 300, want_build="torch")
    assert pb.n_pairs > 0
    # fixed cameras (cameras 10, 11 observed but not optimised)
    fixed = torch.zeros((2, 6), dtype=torch.float64, device=DEV)
    a = same_index(fi, pi, 10, 300, want_build="torch", fixed_cams=fixed)
    assert a.F_fixed == 2
    # an index out of range is refused by both
    for native in (True, False):
        with pytest.raises(ValueError):
            build([0, 12], [0, 1], 12, 300, native)
        with pytest.raises(ValueError):
            build([0, 1], [0, -1], 12, 300, native)


def test_solver_is_bitwise_the_same_with_either_build():
    F, P = 12, 300
    pr = synth.make_ba_problem(F, P, 4, seed=7)
    cams0 = bo.frame_parameters(pr["ext"]).reshape(F, 6)
    out = []
    for native in (True, False):
        pb = ops.BADevice(pr["K"], pr["fi"], pr["pi"], pr["obs"], F, P, DEV, native_index=native)
        assert pb.index_build == ("native" if native else "torch") and pb.n_pairs > 0
        c = torch.as_tensor(cams0.copy()).to(DEV)
        p = torch.as_tensor(pr["pts0"].copy()).to(DEV)
        rep, _ = pb.trf_solve(c, p, 1e-6, 1e-8, 1e-8)
        out.append((c, p, rep.cost, rep.nfev))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and out[0][3] == out[1][3]
