"""GPU: csrc/orb.hip against oracle/orb_oracle.c, bit for bit, on the designed frames of tests/orb_cases.py.

What the rendered frames of tests/test_gpu_parity.py never reach: both rank kernels (sorting and counting, the latter also as
the fallback above 4096 candidates), ties across the select cut and the rank cut, row strides that differ from the width and
widths that are no multiple of 4 (with the padding bytes at 0 and at 255), levels and whole frames without a valid area,
other level counts, scale factors and FAST thresholds, levels without a feature budget, key points on the 31-pixel border and
on the FAST tile seams, a batch of very different frames and a dirty workspace.  tests/test_orb_detect_cpu.py asserts from the
oracle alone that each case contains its edge.  Nothing here has a tolerance.

Run on the MI355X box:  python -m pytest tests/test_orb_detect_gpu.py -q -m gpu
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orb_cases as oc  # noqa: E402
from meatmodeler_amd import ops  # noqa: E402
from meatmodeler_amd._lib import default_context  # noqa: E402
from meatmodeler_amd.orb_pattern import brief_pattern  # noqa: E402
from oracle import orb_oracle as oo  # noqa: E402

DEV = torch.device("cuda", 0)
H, W = oc.H0, oc.W0
RK_MAX = 4096


@pytest.fixture(autouse=True)
def _default_kernels(monkeypatch):
    """Every test starts from the shipped choice of kernels; a test that wants another one sets it itself."""
    monkeypatch.delenv("MM_ORB_RANK", raising=False)
    monkeypatch.delenv("MM_ORB_PYRAMID", raising=False)


def up4(w):
    return (w + 3) // 4 * 4


def pitched(frames, stride=None, fill=0):
    """[B, H, W] host frames as the [B, H, :W] view of a [B, H, stride] device tensor whose other bytes are `fill`."""
    frames = np.asarray(frames)
    B, h, w = frames.shape
    stride = up4(w) if stride is None else stride
    big = np.full((B, h, stride), fill, np.uint8)
    big[:, :, :w] = frames
    view = torch.as_tensor(big).to(DEV)[:, :, :w]
    assert view.stride() == (h * stride, stride, 1)
    return view


def params(nfeatures, nlevels=8, scale_factor=1.2, fast_threshold=20):
    return ops.orb_params(nfeatures, nlevels, scale_factor, 31, fast_threshold)


def detect(view, prm, wsp=None, ws_fill=None):
    B, h, w = view.shape
    if wsp is None:
        wsp = ops.OrbWorkspace(B, h, w, prm, DEV, brief_pattern())
    if ws_fill is not None:
        wsp.ws.fill_(ws_fill)
    wsp.n.fill_(-1)
    out = ops.orb_detect_compute(view, wsp)
    torch.cuda.synchronize()
    return [a.cpu().numpy() for a in out], wsp


def assert_equals_oracle(out, b, r, what=""):
    xy, meta, resp, mom, desc, n = out
    k = r["n"]
    assert n[b] == k, f"{what} frame {b}: key point count {n[b]} vs oracle {k}"
    np.testing.assert_array_equal(meta[b, :k, :4], r["meta"][:, :4], err_msg=f"{what} frame {b} (level, x, y, harris low word)")
    np.testing.assert_array_equal(xy[b, :k], r["xy"], err_msg=f"{what} frame {b} pt")
    np.testing.assert_array_equal(resp[b, :k].view(np.uint32), r["resp"].view(np.uint32), err_msg=f"{what} frame {b} response")
    np.testing.assert_array_equal(mom[b, :k], r["mom"], err_msg=f"{what} frame {b} moments")
    bad = np.nonzero((desc[b, :k] != r["desc"]).any(axis=1))[0]
    assert bad.size == 0, f"{what} frame {b}: {bad.size} descriptors differ, first {bad[:5]}"


def run_case(kind, h, w, nfeatures, **kw):
    out, _ = detect(pitched(oc.frame(kind, h, w)[None]), params(nfeatures, **kw), ws_fill=0xA5)
    assert_equals_oracle(out, 0, oc.reference(kind, h, w, nfeatures, **kw), kind)
    return out


def rank_launch_is_large(view, prm):
    """True if the rank launch of this call had 64 workgroups or more (profile level 2 records only such launches).  With one
    frame the sorting kernel runs nlevels <= 8 workgroups, the counting kernel ceil(kcap / 256) per level."""
    ctx = default_context()
    ctx.profile(2)
    try:
        detect(view, prm)
        names = set(ctx.profile_report())
    finally:
        ctx.profile(0)
    return "orb_rank_kernel" in names


# ---- rank paths --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nfeatures", [500, 300])
@pytest.mark.parametrize("kind", ["dots", "periodic", "noise"])
@pytest.mark.parametrize("rank", ["sort", "count"])
def test_rank_paths_equal_oracle(rank, kind, nfeatures, monkeypatch):
    """Ties across both cuts (dots), equal Harris values with real descriptors (periodic) and a tie-free frame, through the
    sorting and through the counting kernel: each equals the oracle, so they equal each other."""
    monkeypatch.setenv("MM_ORB_RANK", rank)
    run_case(kind, H, W, nfeatures)


@pytest.mark.parametrize("kind", ["dots", "noise"])
def test_capacity_fallback_runs_the_counting_kernel(kind):
    """30000 features: 2 * max(nfeat) + 8 > 4096, so the counting kernel is what runs, with up to 5244 candidates at level 0
    (21 workgroups of a segment work, the others return early).  Both frames come back complete (no level fills its budget)."""
    prm = params(30000)
    nf = ops.orb_level_sizes(H, W, prm)[2]
    assert 2 * int(nf.max()) + 8 > RK_MAX
    assert "MM_ORB_RANK" not in os.environ
    out = run_case(kind, H, W, 30000)
    lvl0 = int((out[1][0, :out[5][0], 0] == 0).sum())
    assert lvl0 == (3400 if kind == "dots" else oc.level_counts(oc.reference("noise", H, W, 30000))[0])
    if kind == "noise":
        assert lvl0 > RK_MAX
        assert rank_launch_is_large(pitched(oc.frame(kind)[None]), prm)


@pytest.mark.parametrize("rank", ["sort", "count"])
def test_complete_survivor_set_below_the_sort_capacity(rank, monkeypatch):
    """150 x 200 at 9000 features: every NMS survivor is kept, 2 * max(nfeat) + 8 <= 4096, levels 5 to 7 have no valid area."""
    monkeypatch.setenv("MM_ORB_RANK", rank)
    prm = params(9000)
    w, h, nf, _ = ops.orb_level_sizes(150, 200, prm)
    assert 2 * int(nf.max()) + 8 <= RK_MAX and (h[5:] <= 62).all()
    out = run_case("noise", 150, 200, 9000)
    assert not (out[1][0, :out[5][0], 0] >= 5).any()


def test_rank_switch_is_read_on_every_call(monkeypatch):
    """MM_ORB_RANK takes effect in a process that has run ORB before.  One frame at 9000 features: the sorting kernel is a launch
    of 8 workgroups, the counting kernel one of 16 x 8."""
    prm = params(9000)
    view = pitched(oc.frame("noise", 150, 200)[None])
    detect(view, prm)                                   # whatever this process did before, it has run ORB now
    assert not rank_launch_is_large(view, prm)          # unset: sort (kcap = 3918 <= 4096)
    monkeypatch.setenv("MM_ORB_RANK", "count")
    assert rank_launch_is_large(view, prm)
    monkeypatch.setenv("MM_ORB_RANK", "sort")
    assert not rank_launch_is_large(view, prm)
    monkeypatch.setenv("MM_ORB_RANK", "count")
    assert rank_launch_is_large(view, prm)
    monkeypatch.delenv("MM_ORB_RANK")
    assert not rank_launch_is_large(view, prm)


# ---- padded strides, widths that are no multiple of 4 --------------------------------------------------------------------

def pyramid_bytes(wsp, B, h0, w0):
    """The pyramid at the head of the workspace: list over levels >= 1 of [B, h, pitch] u8 (zero row padding included)."""
    w, h, _, _ = ops.orb_level_sizes(h0, w0, wsp.prm)
    ws, off, out = wsp.ws.cpu().numpy(), 0, []
    for l in range(1, len(w)):
        pitch = (int(w[l]) + 63) // 64 * 64
        per = (pitch * int(h[l]) + 64 + 255) // 256 * 256
        out.append(np.stack([ws[off + b * per: off + b * per + pitch * int(h[l])].reshape(int(h[l]), pitch) for b in range(B)]))
        off += per * B
    return out, w, h


@pytest.mark.parametrize("pyramid", [None, "levels"])
@pytest.mark.parametrize("extra", [0, 64])
@pytest.mark.parametrize("width", [331, 330, 329])
def test_padding_bytes_reach_no_output(width, extra, pyramid, monkeypatch):
    """Rows `extra` bytes longer than the width rounded up to 4, the bytes behind each row once 0 and once 255: key points,
    descriptors and every pyramid byte are those of the contiguous image.  All survivors are kept (30000 features), so a
    corner that padding creates or suppresses anywhere shows."""
    if pyramid:
        monkeypatch.setenv("MM_ORB_PYRAMID", pyramid)
    kinds = ("noise", "periodic")
    frames = np.stack([oc.frame(k, H, width) for k in kinds])
    prm = params(30000)
    pyr = []
    for fill in (0, 255):
        out, wsp = detect(pitched(frames, up4(width) + extra, fill), prm, ws_fill=0xA5)
        for b, k in enumerate(kinds):
            assert_equals_oracle(out, b, oc.reference(k, H, width, 30000), f"{k} fill {fill}")
        pyr.append(pyramid_bytes(wsp, len(kinds), H, width))
    (p0, w, h), (p255, _, _) = pyr
    prev = frames[0]
    for l in range(1, len(w)):
        np.testing.assert_array_equal(p0[l - 1], p255[l - 1], err_msg=f"level {l}: pyramid bytes depend on the padding")
        assert not p0[l - 1][:, :, int(w[l]):].any()
        prev = oo.resize(prev, int(w[l]), int(h[l]))
        np.testing.assert_array_equal(p0[l - 1][0][:, :int(w[l])], prev, err_msg=f"level {l} against the oracle's resize chain")


# ---- no valid area -------------------------------------------------------------------------------------------------------

def test_frame_without_valid_area_launches_no_fast_kernel():
    prm = params(500)
    w, h, _, _ = ops.orb_level_sizes(62, 64, prm)
    assert ((w <= 62) | (h <= 62)).all()
    view = pitched(np.stack([oc.frame("dots", 62, 64), oc.frame("noise", 62, 64)]))
    ctx = default_context()
    ctx.profile(1)
    try:
        out, _ = detect(view, prm, ws_fill=0xA5)          # (an error code would raise)
        names = set(ctx.profile_report())
    finally:
        ctx.profile(0)
    assert out[5].tolist() == [0, 0]
    assert "orb_fast_kernel" not in names and {"orb_select_kernel", "orb_harris_kernel", "orb_rank_kernel"} <= names


@pytest.mark.parametrize("rank", ["sort", "count"])
def test_one_admissible_pixel(rank, monkeypatch):
    monkeypatch.setenv("MM_ORB_RANK", rank)
    out = run_case("dots", 63, 63, 500)
    assert out[5][0] == 1 and out[1][0, 0, :3].tolist() == [0, 31, 31]


# ---- parameters ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(nlevels=1), dict(nlevels=2), dict(nlevels=5), dict(scale_factor=1.5), dict(scale_factor=1.05),
                                dict(fast_threshold=5), dict(fast_threshold=60)], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_parameters_off_their_defaults(kw):
    run_case("noise", H, W, 400, **kw)


@pytest.mark.parametrize("rank", ["sort", "count"])
@pytest.mark.parametrize("nfeatures", [1, 3])
def test_levels_without_a_feature_budget(nfeatures, rank, monkeypatch):
    monkeypatch.setenv("MM_ORB_RANK", rank)
    nf = ops.orb_level_sizes(H, W, params(nfeatures))[2]
    assert nf.tolist() == ([0, 0, 0, 0, 0, 0, 0, 1] if nfeatures == 1 else [1, 1, 0, 0, 0, 0, 0, 1])
    out = run_case("noise", H, W, nfeatures)
    assert out[5][0] == nfeatures


# ---- batch and workspace hygiene -------------------------------------------------------------------------------------------

def test_mixed_batch_twice_in_one_dirty_workspace():
    kinds = ["dots", "flat", "noise", "periodic"]
    prm = params(500)
    wsp = ops.OrbWorkspace(4, H, W, prm, DEV, brief_pattern())
    wsp.ws.fill_(0xA5)
    for order in (kinds, kinds[::-1]):
        out, _ = detect(pitched(np.stack([oc.frame(k) for k in order])), prm, wsp=wsp)
        for b, k in enumerate(order):
            assert_equals_oracle(out, b, oc.reference(k, H, W, 500), k)
        assert out[5][order.index("flat")] == 0
