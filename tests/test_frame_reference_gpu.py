"""GPU: the per-frame front end -- csrc/flow.hip (pyramid, Lucas-Kanade, Shi-Tomasi) and csrc/contrast.hip (L*a*b*, CLAHE,
grey) -- against oracle/frame_oracle.c at the edges of the kernels: pitches and odd base pointers, images below one tile,
tiles wider than a workgroup and lower than the unrolled trip, row segments of one value, saturated colours, every exit of
the Lucas-Kanade iteration, and the argument errors.

Every comparison is bit for bit; nothing has a tolerance.  The inputs are built by tests/test_frame_reference_cpu.py, which
ties the oracle to the independent restatement oracle/frame_ref.py on the same bytes and asserts what the cases reach.
Buffers written through the raw library calls carry guard bytes, which must come back unchanged.

Run on the MI355X box:  python -m pytest tests/test_frame_reference_gpu.py -q -m gpu
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_frame_reference_cpu as cases  # noqa: E402
from meatmodeler_amd import ops  # noqa: E402
from meatmodeler_amd._lib import MMError, default_context, lib  # noqa: E402
from oracle import frame_oracle as fo  # noqa: E402

DEV = torch.device("cuda", 0)
TABLES = cases.TABLES
FILL = 0xA5


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def filled(n):
    return torch.full((n,), FILL, dtype=torch.uint8, device=DEV)


def pitched(img, pitch, offset):
    """The image as a view with row stride `pitch` whose first byte lies `offset` bytes into a fresh allocation; the bytes
    around it are noise."""
    h, w = img.shape
    assert offset + w <= pitch
    big = np.random.default_rng(pitch).integers(0, 256, (h, pitch), dtype=np.uint8)
    big[:, offset:offset + w] = img
    view = dev(big)[:, offset:offset + w]
    assert view.stride() == (pitch, 1) and view.data_ptr() % 4 == offset % 4
    return view


# ================================================================================================================ pyramid
@pytest.mark.parametrize("w,h", cases.PYR_SIZES)
def test_pyramid_tiny_levels_and_last_tiles(w, h):
    img = cases.pyr_image(w, h)
    got, ref = ops.pyramid(dev(img), cases.PYR_LEVELS), fo.pyramid(img, cases.PYR_LEVELS)
    assert [tuple(t.shape) for t in got] == [a.shape for a in ref]
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(host(a), b)


@pytest.mark.parametrize("w,h", [(131, 35), (129, 33), (3, 5), (1, 1)])
def test_pyr_down_source_pitch_odd_base_and_destination_pitch(w, h):
    ctx = default_context()
    img = cases.pyr_image(w, h)
    ref = fo.pyr_down(img)
    hd, wd = ref.shape
    src = pitched(img, w + 13, 3)
    assert src.data_ptr() % 2 == 1
    dp = wd + 7
    dst = filled((hd + 1) * dp)                                        # one guard row after the last
    ctx.check(lib.mm_pyr_down(ctx.h, src.data_ptr(), w, h, src.stride(0), dst.data_ptr(), dp), "mm_pyr_down")
    out = host(dst).reshape(hd + 1, dp)
    np.testing.assert_array_equal(out[:hd, :wd], ref)
    assert (out[:hd, wd:] == FILL).all() and (out[hd] == FILL).all()


# ============================================================================================= min_eig and good_features
@pytest.mark.parametrize("bs", cases.EIG_BLOCKS)
def test_min_eig_block_sizes_small_images_and_pitch(bs):
    for w, h in cases.EIG_SIZES:
        img = cases.eig_image(w, h)
        ref = fo.min_eig(img, bs)
        np.testing.assert_array_equal(host(ops.min_eig(dev(img), bs)), ref, err_msg=str((w, h)))
    view = pitched(img, w + 9, 5)
    np.testing.assert_array_equal(host(ops.min_eig(view, bs)), ref)


@pytest.mark.parametrize("name", sorted(cases.gftt_images()))
def test_good_features_ties_border_and_distance(name):
    img = cases.gftt_images()[name]
    d = dev(img)
    for bs in cases.GFTT_BLOCKS:
        for mc, q, md in cases.GFTT_PARAMS:
            ref = fo.good_features(img, mc, q, md, bs)
            first, second = ops.good_features(d, mc, q, md, bs), ops.good_features(d, mc, q, md, bs)
            np.testing.assert_array_equal(first, ref, err_msg=str((bs, mc, q, md)))
            np.testing.assert_array_equal(second, first)               # the atomics of the compaction do not show
            assert first.dtype == np.float32 and first.shape == (len(ref), 2)


def test_good_features_without_an_interior_is_empty():
    for w, h in cases.GFTT_TINY:
        got = ops.good_features(dev(cases.noise(w, h, 3)), 0, 0.01, 0.0, 3)
        assert got.shape == (0, 2) and got.dtype == np.float32


# =========================================================================================================== Lucas-Kanade
@functools.lru_cache(maxsize=None)
def _device_pyramids(name, levels):
    a, b = cases.lk_pairs()[name]
    return ops.pyramid(dev(a), levels - 1), ops.pyramid(dev(b), levels - 1)


@pytest.mark.parametrize("win,levels,count,eps", cases.LK_PARAMS)
def test_lk_every_exit(win, levels, count, eps):
    for name, (a, b) in cases.lk_pairs().items():
        pts = cases.lk_points(a.shape[1], a.shape[0], win)
        nx_o, st_o, er_o = fo.lk_track(a, b, pts, win, levels - 1, count, eps)
        pp, pn = _device_pyramids(name, levels)
        nx, st, er = ops.lk_track(pp, pn, dev(pts), win, count, eps)
        np.testing.assert_array_equal(host(st), st_o, err_msg=name)
        np.testing.assert_array_equal(host(nx), nx_o, err_msg=name)
        np.testing.assert_array_equal(host(er), er_o, err_msg=name)


def test_lk_one_point_and_no_point():
    ctx = default_context()
    name, pts, win, levels, count, eps = cases.LK_ONE_POINT
    a, b = cases.lk_pairs()[name]
    pp, pn = _device_pyramids(name, levels)
    pts = np.array(pts, np.float32)
    ref = fo.lk_track(a, b, pts, win, levels - 1, count, eps)
    for x, y in zip(ops.lk_track(pp, pn, dev(pts), win, count, eps), ref):
        np.testing.assert_array_equal(host(x), y)
    nx, st, er = ops.lk_track(pp, pn, torch.zeros((0, 2), dtype=torch.float32, device=DEV))
    assert nx.shape == (0, 2) and st.shape == (0,) and er.shape == (0,)
    # the library itself: n = 0 is a success that reads no argument and launches nothing
    assert lib.mm_lk_track(ctx.h, None, None, None, None, None, 0, None, 0, 0, 0, -1, 0.0, None, None, None) == 0
    ctx.sync()


def test_lk_pitched_level0_and_guarded_outputs():
    ctx = default_context()
    a, b = cases.lk_pairs()["half_flat"]
    h, w = a.shape
    win, levels, count, eps = cases.LK_PARAMS[0]
    pts = cases.lk_points(w, h, win)
    n = len(pts)
    nx_o, st_o, er_o = fo.lk_track(a, b, pts, win, levels - 1, count, eps)
    pyr = []
    for img in (a, b):
        v0 = pitched(img, w + 11, 3)                                   # level 0: a pitched view with an odd base
        l1 = torch.empty(((h + 1) // 2, (w + 1) // 2), dtype=torch.uint8, device=DEV)
        ctx.check(lib.mm_pyr_down(ctx.h, v0.data_ptr(), w, h, v0.stride(0), l1.data_ptr(), l1.stride(0)), "mm_pyr_down")
        pyr.append([v0] + ops.pyramid(l1, levels - 2))
    nx, st, er = ops.lk_track(pyr[0], pyr[1], dev(pts), win, count, eps)
    np.testing.assert_array_equal(host(st), st_o)
    np.testing.assert_array_equal(host(nx), nx_o)
    np.testing.assert_array_equal(host(er), er_o)
    # raw call: outputs with guard elements after n
    g = 16
    out = torch.full((n + g, 2), -777.25, dtype=torch.float32, device=DEV)
    err = torch.full((n + g,), -777.25, dtype=torch.float32, device=DEV)
    sta = filled(n + g)
    L = levels
    arr = lambda xs: (C.c_void_p * L)(*xs)                             # noqa: E731
    ints = lambda xs: (C.c_int * L)(*xs)                               # noqa: E731
    p = dev(pts)
    ctx.check(lib.mm_lk_track(ctx.h, arr([t.data_ptr() for t in pyr[0]]), arr([t.data_ptr() for t in pyr[1]]),
                              ints([t.shape[1] for t in pyr[0]]), ints([t.shape[0] for t in pyr[0]]),
                              ints([t.stride(0) for t in pyr[0]]), L, p.data_ptr(), n, win[0], win[1], count, eps * eps,
                              out.data_ptr(), sta.data_ptr(), err.data_ptr()), "mm_lk_track")
    out, err, sta = host(out), host(err), host(sta)
    np.testing.assert_array_equal(out[:n], nx_o)
    np.testing.assert_array_equal(err[:n], er_o)
    np.testing.assert_array_equal(sta[:n], st_o)
    assert (out[n:] == -777.25).all() and (err[n:] == -777.25).all() and (sta[n:] == FILL).all()


# =============================================================================================================== contrast
@functools.lru_cache(maxsize=None)
def _contrast_oracle(name):
    bgr, clip, tiles = cases.contrast_cases()[name]
    ref = fo.increase_contrast(bgr, TABLES, clip, tiles)
    return ref, fo.bgr_to_grey(ref)


@pytest.mark.parametrize("name", sorted(cases.contrast_cases()))
def test_increase_contrast_paths(name):
    bgr, clip, tiles = cases.contrast_cases()[name]
    ref, ref_grey = _contrast_oracle(name)
    d = dev(bgr[None])
    out, grey = ops.increase_contrast(d, clip, tiles, want_grey=True)
    np.testing.assert_array_equal(host(out)[0], ref)
    np.testing.assert_array_equal(host(grey)[0], ref_grey)
    np.testing.assert_array_equal(host(ops.increase_contrast(d, clip, tiles))[0], ref)             # without the fused grey
    np.testing.assert_array_equal(host(ops.bgr_to_grey(out))[0], ref_grey)


def test_increase_contrast_batch_of_three_odd_frames():
    _, clip, tiles = cases.BATCH_CASE
    imgs = cases.batch_images()
    assert imgs.shape[0] == 3 and (imgs.shape[1] * imgs.shape[2]) % 2 == 1
    out, grey = ops.increase_contrast(dev(imgs), clip, tiles, want_grey=True)
    plain = ops.increase_contrast(dev(imgs), clip, tiles)
    for k, img in enumerate(imgs):
        ref = fo.increase_contrast(img, TABLES, clip, tiles)
        np.testing.assert_array_equal(host(out)[k], ref, err_msg=str(k))
        np.testing.assert_array_equal(host(plain)[k], ref, err_msg=str(k))
        np.testing.assert_array_equal(host(grey)[k], fo.bgr_to_grey(ref), err_msg=str(k))


def _at_offset(data, offset, tail=64):
    """A contiguous device tensor with the bytes of `data`, carved `offset` bytes into a flat buffer filled with FILL."""
    flat = filled(offset + data.size + tail)
    flat[offset:offset + data.size] = dev(data.ravel())
    t = flat[offset:offset + data.size].view(*data.shape)
    assert t.is_contiguous() and t.data_ptr() % 4 == offset % 4
    return flat, t


@pytest.mark.parametrize("name", ["grid_3x5", "seam_100", "17x9"])
def test_increase_contrast_unaligned_buffers(name):
    """An odd bgr base (the dword path of the forward conversion must stand down), then odd output and grey bases as well
    (the dword path of the apply pass), through the raw call with guard bytes around both outputs."""
    ctx = default_context()
    bgr, clip, tiles = cases.contrast_cases()[name]
    ref, ref_grey = _contrast_oracle(name)
    h, w, _ = bgr.shape
    _, src = _at_offset(bgr[None], 1)
    out, grey = ops.increase_contrast(src, clip, tiles, want_grey=True)
    np.testing.assert_array_equal(host(out)[0], ref)
    np.testing.assert_array_equal(host(grey)[0], ref_grey)
    ops.increase_contrast(dev(bgr[None]), clip, tiles)                  # (the tables are on the device now)
    g, cb, gi = ops._LAB_TABLES[str(DEV)]
    ws = torch.empty(lib.mm_contrast_workspace_bytes(1, w, h, tiles[0], tiles[1]), dtype=torch.uint8, device=DEV)
    for o_off, g_off in ((1, 3), (2, 0), (0, 1)):
        oflat, o = _at_offset(np.full((h, w, 3), FILL, np.uint8), 64 + o_off)
        gflat, gr = _at_offset(np.full((h, w), FILL, np.uint8), 64 + g_off)
        ctx.check(lib.mm_increase_contrast(ctx.h, src.data_ptr(), 1, w, h, g.data_ptr(), cb.data_ptr(), gi.data_ptr(), clip,
                                           tiles[0], tiles[1], o.data_ptr(), gr.data_ptr(), ws.data_ptr(), ws.numel()),
                  "mm_increase_contrast")
        np.testing.assert_array_equal(host(o), ref)
        np.testing.assert_array_equal(host(gr), ref_grey)
        for flat, off, size in ((oflat, 64 + o_off, ref.size), (gflat, 64 + g_off, ref_grey.size)):
            f = host(flat)
            assert (f[:off] == FILL).all() and (f[off + size:] == FILL).all()


@pytest.mark.parametrize("n", cases.GREY_COUNTS)
def test_bgr_to_grey_around_one_workgroup(n):
    bgr = cases.grey_row(n)
    flat, src = _at_offset(bgr, 1)
    np.testing.assert_array_equal(host(ops.bgr_to_grey(dev(bgr))), fo.bgr_to_grey(bgr))
    np.testing.assert_array_equal(host(ops.bgr_to_grey(src)), fo.bgr_to_grey(bgr))


# ======================================================================================================== argument errors
def _still_right(ctx):
    """After a refused call the same context computes the right answers."""
    img = cases.eig_image(33, 32)
    np.testing.assert_array_equal(host(ops.min_eig(dev(img), 3, ctx=ctx)), fo.min_eig(img, 3))
    bgr, clip, tiles = cases.contrast_cases()["17x9"]
    np.testing.assert_array_equal(host(ops.increase_contrast(dev(bgr[None]), clip, tiles, ctx=ctx))[0], _contrast_oracle("17x9")[0])
    name, pts, win, levels, count, eps = cases.LK_AFTER_ERROR
    a, b = cases.lk_pairs()[name]
    pts = np.array(pts, np.float32)
    pp, pn = _device_pyramids(name, levels)
    for x, y in zip(ops.lk_track(pp, pn, dev(pts), win, count, eps, ctx=ctx), fo.lk_track(a, b, pts, win, levels - 1, count, eps)):
        np.testing.assert_array_equal(host(x), y)


def _refused(ctx, call):
    with pytest.raises(MMError):
        call()
    _still_right(ctx)


def test_lk_argument_errors():
    ctx = default_context()
    pp, pn = _device_pyramids("tiny", 3)
    pts = dev(np.array([[25.5, 20.25], [10.0, 10.0]], np.float32))
    for win in ((2, 21), (21, 2), (42, 21), (21, 42)):
        _refused(ctx, lambda: ops.lk_track(pp, pn, pts, win, ctx=ctx))
    _refused(ctx, lambda: ops.lk_track([], [], pts, ctx=ctx))                                    # 0 levels
    deep_p, deep_n = _device_pyramids("tiny", 9)
    assert len(deep_p) == 9
    _refused(ctx, lambda: ops.lk_track(deep_p, deep_n, pts, ctx=ctx))                            # 9 levels
    nx, st, er = ops.lk_track(deep_p[:8], deep_n[:8], pts, ctx=ctx)                              # 8 are allowed

    def negative_count():
        L = len(pp)
        arr = lambda xs: (C.c_void_p * L)(*xs)                         # noqa: E731
        ints = lambda xs: (C.c_int * L)(*xs)                           # noqa: E731
        ctx.check(lib.mm_lk_track(ctx.h, arr([t.data_ptr() for t in pp]), arr([t.data_ptr() for t in pn]),
                                  ints([t.shape[1] for t in pp]), ints([t.shape[0] for t in pp]), ints([t.stride(0) for t in pp]),
                                  L, pts.data_ptr(), 2, 21, 21, -1, 1e-4, nx.data_ptr(), st.data_ptr(), er.data_ptr()), "mm_lk_track")
    _refused(ctx, negative_count)


def test_corner_argument_errors():
    ctx = default_context()
    img = dev(cases.eig_image(33, 32))
    for bs in (0, 16):
        _refused(ctx, lambda: ops.min_eig(img, bs, ctx=ctx))
    eig = torch.zeros((5, 2), dtype=torch.float64, device=DEV)
    mx = torch.zeros(1, dtype=torch.int64, device=DEV)
    vb = torch.zeros(16, dtype=torch.int64, device=DEV)
    pos = torch.zeros(16, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    _refused(ctx, lambda: ctx.check(lib.mm_corner_candidates(ctx.h, eig.data_ptr(), 2, 5, 0.01, mx.data_ptr(), vb.data_ptr(),
                                                             pos.data_ptr(), 16, cnt.data_ptr()), "mm_corner_candidates"))


def test_contrast_argument_errors():
    ctx = default_context()
    bgr, clip, tiles = cases.contrast_cases()["17x9"]
    d = dev(bgr[None])
    _refused(ctx, lambda: ops.increase_contrast(d, clip, (18, 1), ctx=ctx))                      # tiles_x = w + 1
    _refused(ctx, lambda: ops.increase_contrast(d, clip, (1, 10), ctx=ctx))                      # tiles_y = h + 1
    _refused(ctx, lambda: ops.increase_contrast(d, 0.0, tiles, ctx=ctx))
    g, cb, gi = ops._LAB_TABLES[str(DEV)]
    need = lib.mm_contrast_workspace_bytes(1, 17, 9, tiles[0], tiles[1])
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(d)

    def run(ws_bytes):
        ctx.check(lib.mm_increase_contrast(ctx.h, d.data_ptr(), 1, 17, 9, g.data_ptr(), cb.data_ptr(), gi.data_ptr(), clip, tiles[0],
                                           tiles[1], out.data_ptr(), None, ws.data_ptr(), ws_bytes), "mm_increase_contrast")
    _refused(ctx, lambda: run(need - 1))                                                         # one byte short
    run(need)
    np.testing.assert_array_equal(host(out)[0], _contrast_oracle("17x9")[0])
