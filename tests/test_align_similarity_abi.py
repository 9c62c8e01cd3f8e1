"""CPU: the symbols of the similarity registration, its argument checks (returned before any device call) and how
mm_align_similarity sizes its workspace (no compute calls)."""
import ctypes as C
import math

import numpy as np
import pytest

ERR_ARG, ERR_WORKSPACE = -1, -3


def lib():
    from meatmodeler_amd import _lib      # (inside the tests, as in test_abi.py: not while the suite is being collected)
    return _lib


def size(n_prob, n_hyp, N):
    return lib().lib.mm_align_workspace_bytes(n_prob, n_hyp, N)


def test_library_table_has_the_align_symbols():
    _lib = lib()
    for name in ("mm_align_workspace_bytes", "mm_align_similarity", "mm_apply_similarity", "mm_camera_centres"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert C.sizeof(_lib.AlignParams) == 6 * 4 + 2 * 4 + 2 * 8      # matches sizeof(mm_align_params)
    assert _lib.lib.mm_abi_version() == 3
    from meatmodeler_amd import ops, processor, pipeline
    assert (ops.ALIGN_TOO_FEW, ops.ALIGN_NO_MODEL, ops.ALIGN_WEAK, ops.ALIGN_NONFINITE) == (1, 2, 4, 8)
    assert callable(ops.align_similarity) and callable(ops.apply_similarity) and callable(ops.camera_centres)
    assert callable(processor.alignSimilarity) and callable(processor.applySimilarity) and callable(pipeline.align_options)


def call(prm, ptr=(0, 10), n_prob=None, ws_bytes=None, null=(), ctx=None):
    """mm_align_similarity without a context and with pointers nothing is read through (1 stands for a device address)."""
    _lib = lib()
    ph = np.asarray(ptr, np.int64)
    n_prob = len(ph) - 1 if n_prob is None else n_prob
    p = {k: (None if k in null else 1) for k in ("src", "dst", "sim", "cost", "inlier", "info", "ws")}
    if ws_bytes is None:
        ws_bytes = size(max(n_prob, 0), prm.n_hyp if prm is not None else 1, int(ph[-1]))
    return _lib.lib.mm_align_similarity(ctx, p["src"], p["dst"], None if "ptr" in null else ph.ctypes.data_as(_lib.c_i64p), n_prob,
                                        None if prm is None else C.byref(prm), p["sim"], p["cost"], p["inlier"], p["info"], p["ws"],
                                        ws_bytes)


def params(**kw):
    f = dict(n_hyp=256, min_points=3, min_inliers=3, refit_iters=2, with_scale=1, reserved=0, seed=0, prob_base=0, tau=0.1,
             collinear_tol=1e-6)
    f.update(kw)
    return lib().AlignParams(*[f[k] for k in ("n_hyp", "min_points", "min_inliers", "refit_iters", "with_scale", "reserved", "seed",
                                              "prob_base", "tau", "collinear_tol")])


BAD_PARAMS = [dict(n_hyp=0), dict(n_hyp=4097), dict(n_hyp=-1), dict(tau=0.0), dict(tau=-1.0), dict(tau=math.nan), dict(tau=math.inf),
              dict(collinear_tol=-1e-6), dict(collinear_tol=math.nan), dict(refit_iters=-1), dict(refit_iters=1001),
              dict(min_inliers=-1), dict(with_scale=2)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_bad_parameters_return_err_arg_before_the_workspace_is_judged(bad):
    # a workspace of 0 bytes would be MM_ERR_WORKSPACE: the argument error comes first, and neither needs a context
    assert call(params(**bad), ws_bytes=0) == ERR_ARG


@pytest.mark.parametrize("ptr", [(0, 5, 4), (-1, 5), (3, 2), (0, 1 << 31)])
def test_bad_ptr_returns_err_arg(ptr):
    assert call(params(), ptr=ptr, ws_bytes=0) == ERR_ARG


@pytest.mark.parametrize("null", ["ptr", "src", "dst", "sim", "cost", "inlier", "info", "ws"])
def test_null_pointers_return_err_arg(null):
    assert call(params(), null=(null,), ws_bytes=0) == ERR_ARG


def test_null_params_and_negative_count_return_err_arg():
    assert call(None, ws_bytes=0) == ERR_ARG
    assert call(params(), n_prob=-1, ws_bytes=0) == ERR_ARG


def test_workspace_too_small_returns_err_workspace_without_a_device():
    need = size(1, 256, 10)
    assert call(params(), ws_bytes=need - 1) == ERR_WORKSPACE and call(params(), ws_bytes=0) == ERR_WORKSPACE
    # a sufficient one passes every check and stops at the missing context
    assert call(params(), ws_bytes=need) == ERR_ARG
    many = (0, 4097, 4097, 4100, 4400)
    assert call(params(n_hyp=65), ptr=many, ws_bytes=size(4, 65, 4400) - 1) == ERR_WORKSPACE
    # src, dst and inlier may be null when no problem has a row; n_prob = 0 needs no buffer at all
    assert call(params(), ptr=(0, 0, 0), null=("src", "dst", "inlier")) == ERR_ARG
    assert call(params(), ptr=(0,), null=("src", "dst", "sim", "cost", "inlier", "info", "ws"), ws_bytes=0) == ERR_ARG


def test_apply_and_centres_argument_errors():
    L = lib().lib
    assert L.mm_apply_similarity(None, None, 1, 4, 1, 4) == ERR_ARG
    assert L.mm_apply_similarity(None, 1, 1, -1, 1, 4) == ERR_ARG and L.mm_apply_similarity(None, 1, 1, 4, 1, -1) == ERR_ARG
    assert L.mm_camera_centres(None, None, 3, 1) == ERR_ARG and L.mm_camera_centres(None, 1, 3, None) == ERR_ARG
    assert L.mm_camera_centres(None, 1, -1, 1) == ERR_ARG


def test_workspace_grows_with_each_argument():
    assert size(1, 256, 5000) > 0 and size(1, 256, 5000) % 256 == 0
    assert size(2, 256, 5000) > size(1, 256, 5000)
    assert size(1, 512, 5000) > size(1, 256, 5000)
    assert size(1, 256, 50000) > size(1, 256, 5000)
    assert size(-1, 256, 10) == size(0, 256, 10) and size(1, -4, 10) == size(1, 0, 10) and size(1, 8, -10) == size(1, 8, 0)
    # it holds the hypotheses (13 doubles each), a partial cost per (chunk, hypothesis) and a cost per hypothesis
    chunks = 600000 // 4096 + 1
    assert size(1, 256, 600000) >= 8 * 256 * (13 + chunks + 1)
    assert size(1, 256, 600000) <= 8 * 256 * (13 + chunks + 1) + 8 * 20 * chunks + 4 * chunks + 8 * 40 + 16 + 7 * 256


def test_ops_reject_bad_arguments_before_any_device_call():
    import torch
    from meatmodeler_amd import ops
    a = torch.zeros((5, 3), dtype=torch.float64)
    for kw in (dict(), dict(tau=0.1, tau_rel=0.1), dict(tau=0.0), dict(tau=0.1, n_hyp=0), dict(tau=0.1, ptr=[0, 3, 2]),
               dict(tau=0.1, ptr=[0, 9]), dict(tau_rel=0.1, ptr=[0, 2, 5]), dict(tau=0.1, refit_iters=-1), dict(tau_rel=-1.0)):
        with pytest.raises(ValueError):
            ops.align_similarity(a, a, **kw)
    with pytest.raises(ValueError):
        ops.align_similarity(a, a[:4], tau=0.1)
    with pytest.raises(ValueError):
        ops.align_similarity(a.float(), a.float(), tau=0.1)
    with pytest.raises(ValueError):
        ops.apply_similarity(torch.zeros(12, dtype=torch.float64), a)
    with pytest.raises(ValueError):
        ops.camera_centres(torch.zeros((2, 4, 4), dtype=torch.float64))
