"""CPU: the symbols of the observation filter, its argument checks (returned before any device call), how
mm_filter_observations sizes its workspace, and what ops.filter_observations and pipeline.refine_options refuse (no compute
calls, no context)."""
import ctypes as C
import math

import numpy as np
import pytest

ERR_ARG, ERR_WORKSPACE = -1, -3
K_OK = (800.0, 0.0, 320.0, 0.0, 800.0, 240.0, 0.0, 0.0, 1.0)
POINTERS = ("cams", "pts", "fi", "pi", "obs", "pt_ptr", "obs_flags", "err", "depth", "pt_flags", "cos_parallax", "fi_out", "pi_out",
            "obs_out", "obs_map", "point_map", "counts", "ws")


def lib():
    from meatmodeler_amd import _lib      # (inside the tests, as in test_abi.py: not while the suite is being collected)
    return _lib


def size(F, P, O):
    return lib().lib.mm_filter_workspace_bytes(F, P, O)


def params(**kw):
    f = dict(min_views=2, reserved=0, max_reproj_px=4.0, min_depth=0.0, max_cos_parallax=2.0)
    f.update(kw)
    return lib().FilterParams(*[f[k] for k in ("min_views", "reserved", "max_reproj_px", "min_depth", "max_cos_parallax")])


def call(prm, F=4, P=10, O=30, K=K_OK, ws_bytes=None, null=()):
    """mm_filter_observations without a context and with pointers nothing is read through (16 stands for a device address)."""
    _lib = lib()
    p = {k: (None if k in null else 16) for k in POINTERS}
    Kh = None if K is None else np.asarray(K, np.float64)
    if ws_bytes is None:
        ws_bytes = size(F, P, O)
    return _lib.lib.mm_filter_observations(None, p["cams"], F, p["pts"], P, None if Kh is None else Kh.ctypes.data_as(_lib.c_f64p),
                                           p["fi"], p["pi"], p["obs"], O, p["pt_ptr"], None if prm is None else C.byref(prm),
                                           p["obs_flags"], p["err"], p["depth"], p["pt_flags"], p["cos_parallax"], p["fi_out"],
                                           p["pi_out"], p["obs_out"], p["obs_map"], p["point_map"], p["counts"], p["ws"], ws_bytes)


def test_library_table_has_the_filter_symbols():
    _lib = lib()
    for name in ("mm_filter_workspace_bytes", "mm_filter_observations"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert C.sizeof(_lib.FilterParams) == 2 * 4 + 3 * 8      # matches sizeof(mm_filter_params)
    assert _lib.lib.mm_abi_version() == 3
    from meatmodeler_amd import bundleAdjuster, ops, pipeline
    assert (ops.OBS_REPROJ, ops.OBS_BEHIND, ops.OBS_NONFINITE, ops.OBS_ORPHAN) == (1, 2, 4, 8)
    assert (ops.PT_SHORT, ops.PT_PARALLAX, ops.PT_NONFINITE) == (1, 2, 4) and ops.FILTER_CHUNK == 1024
    assert callable(ops.filter_observations) and callable(pipeline.refine_options)
    assert callable(bundleAdjuster.filterPoints) and callable(bundleAdjuster.refinePoints)
    # the header's constants are the ones the wrappers and the restatement use
    import os
    import re
    import test_filter_observations_cpu as ref
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "meatmodeler.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (MM_(?:OBS|PT|FILTER)_[A-Z]+) (\d+)", src)}
    assert defs == dict(MM_OBS_REPROJ=1, MM_OBS_BEHIND=2, MM_OBS_NONFINITE=4, MM_OBS_ORPHAN=8, MM_PT_SHORT=1, MM_PT_PARALLAX=2,
                        MM_PT_NONFINITE=4, MM_FILTER_CHUNK=ops.FILTER_CHUNK)
    assert ref.CHUNK == ops.FILTER_CHUNK


BAD_PARAMS = [dict(min_views=1), dict(min_views=0), dict(min_views=-3), dict(max_reproj_px=math.nan), dict(min_depth=math.nan),
              dict(max_cos_parallax=math.nan)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_bad_parameters_return_err_arg_before_the_workspace_is_judged(bad):
    # a workspace of 0 bytes would be MM_ERR_WORKSPACE: the argument error comes first, and neither needs a context
    assert call(params(**bad), ws_bytes=0) == ERR_ARG


def test_thresholds_that_switch_a_test_off_are_arguments_like_any_other():
    off = params(max_reproj_px=math.inf, min_depth=-math.inf, max_cos_parallax=2.0)
    assert call(off, ws_bytes=0) == ERR_WORKSPACE


@pytest.mark.parametrize("K", [None, (800.0, 0, 320, 0, 800, 240, 0, 0, 2.0), (800.0, 0, 320, 1e-3, 800, 240, 0, 0, 1),
                               (800.0, 0, 320, 0, 800, 240, 1e-9, 0, 1), (800.0, 0, 320, 0, 800, 240, 0, 1e-9, 1),
                               (0.0, 0, 320, 0, 800, 240, 0, 0, 1), (800.0, 0, 320, 0, 0.0, 240, 0, 0, 1),
                               (800.0, math.nan, 320, 0, 800, 240, 0, 0, 1), (800.0, 0, math.inf, 0, 800, 240, 0, 0, 1)])
def test_a_k_the_resection_would_refuse_returns_err_arg(K):
    assert call(params(), K=K, ws_bytes=0) == ERR_ARG


@pytest.mark.parametrize("null", POINTERS)
def test_null_pointers_return_err_arg(null):
    assert call(params(), null=(null,), ws_bytes=0) == ERR_ARG


def test_null_params_and_bad_sizes_return_err_arg():
    assert call(None, ws_bytes=0) == ERR_ARG
    for kw in (dict(F=-1), dict(P=-1), dict(O=-1), dict(F=0), dict(O=1 << 31), dict(P=(1 << 31) - 1, O=5)):
        assert call(params(), ws_bytes=0, **kw) == ERR_ARG, kw


def test_workspace_too_small_returns_err_workspace_without_a_device():
    need = size(4, 10, 30)
    assert call(params(), ws_bytes=need - 1) == ERR_WORKSPACE and call(params(), ws_bytes=0) == ERR_WORKSPACE
    # a sufficient one passes every check and stops at the missing context
    assert call(params(), ws_bytes=need) == ERR_ARG
    assert call(params(), F=300, P=70000, O=400000, ws_bytes=size(300, 70000, 400000) - 1) == ERR_WORKSPACE
    # without observations or without points only counts is written: no other buffer is needed, and no workspace
    rest = tuple(k for k in POINTERS if k != "counts")
    assert call(params(), O=0, null=rest, ws_bytes=0) == ERR_ARG and call(params(), P=0, O=0, F=0, null=rest, ws_bytes=0) == ERR_ARG
    assert call(params(), O=0, null=("counts",), ws_bytes=0) == ERR_ARG


def test_workspace_grows_with_each_argument():
    base = size(100, 5000, 20000)
    assert base > 0 and base % 256 == 0
    assert size(200, 5000, 20000) > base and size(100, 6000, 20000) > base and size(100, 5000, 200000) > base
    assert size(-1, 10, 10) == size(0, 10, 10) and size(1, -4, 10) == size(1, 0, 10) and size(1, 8, -10) == size(1, 8, 0)
    # the camera table (15 doubles a camera), a new index per point and three sums per chunk
    chunks = lambda n: -(-n // 1024)
    F, P, O = 500, 400000, 2000000
    body = 8 * 15 * F + 4 * P + 4 * (2 * chunks(O) + chunks(P))
    assert body <= size(F, P, O) <= body + 5 * 256


def tensors(F=4, P=6, per=3):
    import torch
    fi = torch.arange(P * per, dtype=torch.int32) % F
    pi = torch.arange(P * per, dtype=torch.int32) // per
    return dict(cams=torch.zeros((F, 6), dtype=torch.float64), pts=torch.ones((P, 3), dtype=torch.float64),
                K=np.asarray(K_OK).reshape(3, 3), fi=fi, pi=pi, obs=torch.zeros((P * per, 2), dtype=torch.float64))


def test_ops_reject_bad_arguments_before_any_device_call():
    import torch
    from meatmodeler_amd import ops
    good = tensors()

    def refuses(tests=None, **change):
        a = dict(good, **change)
        with pytest.raises(ValueError):
            ops.filter_observations(a["cams"], a["pts"], a["K"], a["fi"], a["pi"], a["obs"], a.get("pt_ptr"),
                                    **(dict(max_reproj_px=4.0) if tests is None else tests))

    # no active test at all, and thresholds the library would refuse
    for tests in ({}, dict(min_views=2), dict(max_reproj_px=math.nan), dict(min_depth=math.nan), dict(max_reproj_px=4.0, min_views=1),
                  dict(min_angle_deg=-1.0), dict(min_angle_deg=math.nan), dict(max_reproj_px=4.0, min_views=2.5)):
        refuses(tests=tests)
    # shapes and dtypes
    refuses(cams=good["cams"][:, :5])
    refuses(pts=good["pts"].float())
    refuses(pts=good["pts"].reshape(-1))
    refuses(fi=good["fi"].long())
    refuses(pi=good["pi"][:-1])
    refuses(obs=good["obs"].float())
    refuses(obs=good["obs"][:, :1])
    refuses(pt_ptr=torch.zeros(5, dtype=torch.int32))
    refuses(pt_ptr=torch.zeros(7, dtype=torch.int64))
    refuses(K=np.eye(3) * 2.0)
    refuses(K=np.zeros(8))
    # indices out of range, observations that are not point-major, a pt_ptr that is not their CSR
    refuses(fi=good["fi"] + 1)
    refuses(fi=good["fi"] - 1)
    refuses(pi=good["pi"] + 1)
    refuses(pi=good["pi"].flip(0))
    refuses(pt_ptr=torch.tensor([0, 3, 6, 9, 12, 15, 17], dtype=torch.int32))
    refuses(pt_ptr=torch.tensor([0, 3, 6, 5, 12, 15, 18], dtype=torch.int32))
    refuses(pts=good["pts"][:0])


def test_refine_options_refuse_bad_input():
    from meatmodeler_amd.pipeline import refine_options
    assert refine_options(None) is None
    d = refine_options({})
    assert d["rounds"] == 2 and len(d["max_reproj_px"]) == 2 and d["max_reproj_px"][0] > d["max_reproj_px"][1] and d["ftol"] == 1e-4
    assert d["max_nfev"] is None
    # one threshold per round, the last one repeated
    assert refine_options(dict(max_reproj_px=(16, 8, 4), rounds=5))["max_reproj_px"] == [16.0, 8.0, 4.0, 4.0, 4.0]
    assert refine_options(dict(max_reproj_px=3, rounds=1, min_views=3, max_nfev=7)) == dict(max_reproj_px=[3.0], rounds=1, ftol=1e-4,
                                                                                            max_nfev=7, min_views=3)
    for bad in ("yes", 4.0, dict(max_reproj=4.0), dict(rounds=0), dict(rounds=1.5), dict(rounds=True), dict(max_reproj_px=()),
                dict(max_reproj_px="wide"), dict(max_reproj_px=math.nan), dict(max_reproj_px=(8.0, math.nan)),
                dict(max_reproj_px=math.inf), dict(min_views=1), dict(min_angle_deg=-2.0), dict(min_depth=math.nan), dict(ftol=0.0),
                dict(ftol=-1e-4), dict(max_nfev=0), dict(max_nfev=2.5)):
        with pytest.raises(ValueError):
            refine_options(bad)
    # a wide first round may be switched off as long as some test stays active
    assert refine_options(dict(max_reproj_px=math.inf, min_depth=0.0))["max_reproj_px"] == [math.inf, math.inf]
