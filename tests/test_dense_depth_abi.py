"""CPU: the symbols of the dense depth stage, their argument checks (returned before any device call), how mm_depth_sweep and
mm_depth_fuse size their workspaces, and what ops.depth_sweep and ops.depth_fuse refuse (no compute calls, no context)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ERR_ARG, ERR_WORKSPACE = -1, -3
K_OK = (800.0, 0.0, 320.0, 0.0, 800.0, 240.0, 0.0, 0.0, 1.0)
BAD_K = [None, (800.0, 0, 320, 0, 800, 240, 0, 0, 2.0), (800.0, 0, 320, 1e-3, 800, 240, 0, 0, 1), (800.0, 0, 320, 0, 800, 240, 1e-9, 0, 1),
         (800.0, 0, 320, 0, 800, 240, 0, 1e-9, 1), (0.0, 0, 320, 0, 800, 240, 0, 0, 1), (800.0, 0, 320, 0, 0.0, 240, 0, 0, 1),
         (800.0, math.nan, 320, 0, 800, 240, 0, 0, 1), (800.0, 0, math.inf, 0, 800, 240, 0, 0, 1)]
SWEEP_POINTERS = ("img", "ref", "src", "AB", "w0", "dw", "depth", "cost", "plane", "ws")
FUSE_POINTERS = ("depth", "cost", "ext", "nbr", "grey", "points", "grey_out", "origin", "n_consistent", "keep", "counts", "ws")


def lib():
    from meatmodeler_amd import _lib      # (inside the tests, as in test_abi.py: not while the suite is being collected)
    return _lib


def sweep_params(**kw):
    f = dict(planes=64, radius=3, min_sources=1, reserved=0, var_min=4.0)
    f.update(kw)
    return lib().SweepParams(*[f[k] for k in ("planes", "radius", "min_sources", "reserved", "var_min")])


def fuse_params(**kw):
    f = dict(min_consistent=2, reserved=0, max_cost=0.4, eps_depth=0.01, tau_px=1.0)
    f.update(kw)
    return lib().FuseParams(*[f[k] for k in ("min_consistent", "reserved", "max_cost", "eps_depth", "tau_px")])


def host_K(K):
    return None if K is None else np.asarray(K, np.float64)


def sweep_call(prm, F=7, H=120, W=160, V=5, S=4, K=K_OK, ws_bytes=None, null=()):
    """mm_depth_sweep without a context and with pointers nothing is read through (16 stands for a device address)."""
    _lib = lib()
    p = {k: (None if k in null else 16) for k in SWEEP_POINTERS}
    Kh = host_K(K)
    if ws_bytes is None:
        ws_bytes = _lib.lib.mm_depth_sweep_workspace_bytes(V, S, prm.planes if prm is not None else 1)
    return _lib.lib.mm_depth_sweep(None, p["img"], F, H, W, None if Kh is None else Kh.ctypes.data_as(_lib.c_f64p), p["ref"], p["src"], p["AB"],
                                   p["w0"], p["dw"], V, S, None if prm is None else C.byref(prm), p["depth"], p["cost"], p["plane"], p["ws"],
                                   ws_bytes)


def fuse_call(prm, V=5, H=120, W=160, Q=4, K=K_OK, cap=1000, ws_bytes=None, null=()):
    _lib = lib()
    p = {k: (None if k in null else 16) for k in FUSE_POINTERS}
    Kh = host_K(K)
    if ws_bytes is None:
        ws_bytes = _lib.lib.mm_depth_fuse_workspace_bytes(V, H, W)
    return _lib.lib.mm_depth_fuse(None, p["depth"], p["cost"], V, H, W, p["ext"], None if Kh is None else Kh.ctypes.data_as(_lib.c_f64p),
                                  p["nbr"], Q, p["grey"], None if prm is None else C.byref(prm), cap, p["points"], p["grey_out"], p["origin"],
                                  p["n_consistent"], p["keep"], p["counts"], p["ws"], ws_bytes)


def test_library_table_has_the_dense_symbols():
    _lib = lib()
    for name in ("mm_depth_sweep_workspace_bytes", "mm_depth_sweep", "mm_depth_fuse_workspace_bytes", "mm_depth_fuse"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert C.sizeof(_lib.SweepParams) == 4 * 4 + 8 and C.sizeof(_lib.FuseParams) == 2 * 4 + 3 * 8      # sizeof(mm_sweep_params), (mm_fuse_params)
    assert _lib.lib.mm_abi_version() == 3
    from meatmodeler_amd import ops, pipeline, processor
    assert callable(ops.depth_sweep) and callable(ops.depth_fuse) and callable(ops.sweep_tables)
    assert callable(pipeline.dense_options) and callable(pipeline.ClipPipeline.dense) and callable(processor.densePointCloud)
    # the header's constants are the ones the wrappers use
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "meatmodeler.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (MM_(?:SWEEP|FUSE)_[A-Z_]+) (\d+)", src)}
    assert defs == dict(MM_SWEEP_TILE=ops.SWEEP_TILE, MM_SWEEP_MAX_RADIUS=ops.SWEEP_MAX_RADIUS, MM_SWEEP_MAX_PLANES=ops.SWEEP_MAX_PLANES,
                        MM_SWEEP_MAX_SOURCES=ops.SWEEP_MAX_SOURCES, MM_FUSE_MAX_NEIGHBOURS=ops.FUSE_MAX_NEIGHBOURS)
    assert ops.SWEEP_TILE == 16
    import test_dense_depth_cpu as ref
    assert ref.CHUNK == ops.FILTER_CHUNK


# ------------------------------------------------------------------------------------------------ mm_depth_sweep

BAD_SWEEP = [dict(planes=0), dict(planes=-2), dict(planes=4097), dict(radius=0), dict(radius=5), dict(min_sources=0), dict(min_sources=5),
             dict(var_min=-1.0), dict(var_min=math.nan), dict(var_min=math.inf)]


@pytest.mark.parametrize("bad", BAD_SWEEP, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_bad_sweep_parameters_return_err_arg_before_the_workspace_is_judged(bad):
    # a workspace of 0 bytes would be MM_ERR_WORKSPACE: the argument error comes first, and neither needs a context
    assert sweep_call(sweep_params(**bad), ws_bytes=0) == ERR_ARG


@pytest.mark.parametrize("K", BAD_K)
def test_the_sweep_refuses_a_k_the_resection_would_refuse(K):
    assert sweep_call(sweep_params(), K=K, ws_bytes=0) == ERR_ARG


@pytest.mark.parametrize("null", SWEEP_POINTERS)
def test_the_sweep_refuses_null_pointers(null):
    assert sweep_call(sweep_params(), null=(null,), ws_bytes=0) == ERR_ARG


def test_the_sweep_refuses_null_params_and_bad_sizes():
    assert sweep_call(None, ws_bytes=0) == ERR_ARG
    for kw in (dict(F=0), dict(F=-1), dict(H=0), dict(W=-3), dict(V=-1), dict(S=0), dict(S=17), dict(V=65536, H=8, W=8),
               dict(F=70000, H=200, W=200), dict(V=60000, H=200, W=200)):
        assert sweep_call(sweep_params(), ws_bytes=0, **kw) == ERR_ARG, kw


def test_the_sweep_workspace():
    _lib = lib()
    size = _lib.lib.mm_depth_sweep_workspace_bytes
    need = size(5, 4, 64)
    assert need % 256 == 0 and 5 * 4 * 64 * 3 * 8 <= need < 5 * 4 * 64 * 3 * 8 + 256
    assert size(6, 4, 64) > need and size(5, 5, 64) > need and size(5, 4, 80) > need
    assert size(-1, 4, 64) == size(0, 4, 64) == 0 and size(5, -4, 64) == 0 and size(5, 4, -1) == 0
    assert sweep_call(sweep_params(), ws_bytes=need - 1) == ERR_WORKSPACE and sweep_call(sweep_params(), ws_bytes=0) == ERR_WORKSPACE
    # a sufficient one passes every check and stops at the missing context
    assert sweep_call(sweep_params(), ws_bytes=need) == ERR_ARG
    # an image without a single window is an argument like any other: the workspace is still judged
    assert sweep_call(sweep_params(), H=5, W=5, ws_bytes=0) == ERR_WORKSPACE
    # without views nothing is written: no buffer is needed, and no workspace
    assert sweep_call(sweep_params(), V=0, null=SWEEP_POINTERS, ws_bytes=0) == ERR_ARG
    assert sweep_call(sweep_params(planes=0), V=0, null=SWEEP_POINTERS, ws_bytes=0) == ERR_ARG


# ------------------------------------------------------------------------------------------------ mm_depth_fuse

BAD_FUSE = [dict(max_cost=math.nan), dict(eps_depth=-0.01), dict(eps_depth=math.nan), dict(tau_px=-1.0), dict(tau_px=math.nan),
            dict(min_consistent=-1)]


@pytest.mark.parametrize("bad", BAD_FUSE, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_bad_fuse_parameters_return_err_arg_before_the_workspace_is_judged(bad):
    assert fuse_call(fuse_params(**bad), ws_bytes=0) == ERR_ARG


def test_fuse_thresholds_that_switch_a_test_off_are_arguments_like_any_other():
    off = fuse_params(max_cost=math.inf, eps_depth=math.inf, tau_px=math.inf, min_consistent=0)
    assert fuse_call(off, ws_bytes=0) == ERR_WORKSPACE
    assert fuse_call(fuse_params(max_cost=-math.inf), ws_bytes=0) == ERR_WORKSPACE


@pytest.mark.parametrize("K", BAD_K)
def test_the_fuse_refuses_a_k_the_resection_would_refuse(K):
    assert fuse_call(fuse_params(), K=K, ws_bytes=0) == ERR_ARG


@pytest.mark.parametrize("null", FUSE_POINTERS)
def test_the_fuse_refuses_null_pointers(null):
    assert fuse_call(fuse_params(), null=(null,), ws_bytes=0) == ERR_ARG


def test_the_fuse_refuses_null_params_and_bad_sizes():
    assert fuse_call(None, ws_bytes=0) == ERR_ARG
    for kw in (dict(V=-1), dict(H=0), dict(W=0), dict(Q=-1), dict(Q=65), dict(cap=-1), dict(V=60000, H=200, W=200)):
        assert fuse_call(fuse_params(), ws_bytes=0, **kw) == ERR_ARG, kw


def test_the_fuse_workspace():
    _lib = lib()
    size = _lib.lib.mm_depth_fuse_workspace_bytes
    need = size(5, 120, 160)
    chunks = -(-5 * 120 * 160 // 1024)
    assert need % 256 == 0 and 5 * 120 * 160 + 2 * 4 * chunks <= need <= 5 * 120 * 160 + 2 * 4 * chunks + 3 * 256
    assert size(6, 120, 160) > need and size(5, 121, 160) > need and size(5, 120, 161) > need
    assert size(0, 120, 160) == size(-1, 120, 160) == size(5, 0, 160) == size(5, 120, -1) == 0
    assert fuse_call(fuse_params(), ws_bytes=need - 1) == ERR_WORKSPACE and fuse_call(fuse_params(), ws_bytes=0) == ERR_WORKSPACE
    assert fuse_call(fuse_params(), ws_bytes=need) == ERR_ARG                  # every check passed: the missing context
    # the neighbour table may be missing when it has no columns, the row outputs when there are no rows
    assert fuse_call(fuse_params(), Q=0, null=("nbr",), ws_bytes=0) == ERR_WORKSPACE
    assert fuse_call(fuse_params(), cap=0, null=("points", "grey_out", "origin", "n_consistent"), ws_bytes=0) == ERR_WORKSPACE
    # without views only counts is written
    rest = tuple(k for k in FUSE_POINTERS if k != "counts")
    assert fuse_call(fuse_params(), V=0, null=rest, ws_bytes=0) == ERR_ARG
    assert fuse_call(fuse_params(), V=0, null=("counts",), ws_bytes=0) == ERR_ARG


# ------------------------------------------------------------------------------------------------ the wrappers

def sweep_inputs():
    import torch
    F, H, W = 4, 20, 24
    ext = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (F, 1, 1))
    ext[:, 0, 3] = np.arange(F) * 0.1
    return dict(img=torch.zeros((F, H, W), dtype=torch.uint8), K=np.asarray(K_OK).reshape(3, 3), extrinsics=ext, ref=[1, 2],
                src=[[0, 2], [1, 3]], ranges=[[4.0, 9.0], [4.0, 9.0]])


def test_depth_sweep_rejects_bad_arguments_before_any_device_call():
    import torch
    from meatmodeler_amd import ops
    good = sweep_inputs()

    def refuses(**change):
        with pytest.raises(ValueError):
            ops.depth_sweep(**dict(good, **change))

    refuses(img=good["img"].float())
    refuses(img=good["img"][0])
    refuses(img=good["img"].numpy())
    refuses(extrinsics=good["extrinsics"][:3])
    refuses(extrinsics=good["extrinsics"][:, :, :3])
    refuses(K=np.eye(3) * 2.0)
    refuses(ref=[4, 1])
    refuses(ref=[1])
    refuses(src=[[0, 4], [1, 3]])
    refuses(src=[[0, 2, 3], [1, 3]])
    refuses(src=[0, 2])
    refuses(ranges=[[4.0, 9.0]])
    refuses(ranges=[[0.0, 9.0], [4.0, 9.0]])
    refuses(ranges=[[4.0, math.nan], [4.0, 9.0]])
    for kw in (dict(planes=0), dict(planes=4097), dict(planes=8.5), dict(radius=0), dict(radius=5), dict(radius="wide"), dict(min_sources=0),
               dict(min_sources=3), dict(var_min=-1.0), dict(var_min=math.nan), dict(var_min=None)):
        refuses(**kw)


def test_depth_fuse_rejects_bad_arguments_before_any_device_call():
    import torch
    from meatmodeler_amd import ops
    V, H, W = 3, 10, 12
    ext = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (V, 1, 1))
    good = dict(depth=torch.ones((V, H, W)), cost=torch.zeros((V, H, W)), K=np.asarray(K_OK).reshape(3, 3), extrinsics=ext,
                nbr=[[1, 2], [0, 2], [0, 1]], grey=torch.zeros((V, H, W), dtype=torch.uint8))

    def refuses(**change):
        with pytest.raises(ValueError):
            ops.depth_fuse(**dict(good, **change))

    refuses(depth=good["depth"].double())
    refuses(cost=good["cost"][:2])
    refuses(grey=good["grey"].float())
    refuses(grey=good["grey"][:, :5])
    refuses(K=np.zeros(8))
    refuses(extrinsics=ext[:2])
    refuses(nbr=[[1, 2], [0, 2]])
    refuses(nbr=[[1, 3], [0, 2], [0, 1]])
    refuses(nbr=[[0, 2], [0, 2], [0, 1]])               # a view is not its own neighbour
    refuses(nbr=[[-2, 2], [0, 2], [0, 1]])
    refuses(nbr=[1, 0, 0])
    for kw in (dict(max_cost=math.nan), dict(eps_depth=-0.1), dict(tau_px=math.nan), dict(min_consistent=-1), dict(min_consistent=1.5),
               dict(cap=-1), dict(max_cost="low")):
        refuses(**kw)
