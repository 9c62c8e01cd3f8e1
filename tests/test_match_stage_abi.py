"""CPU: how mm_bf_match_ratio_batched carves its workspace (no compute calls)."""
import pytest


def up(x):
    return (x + 255) // 256 * 256


def sizes(n_pairs, nq_cap, nt_cap):
    from meatmodeler_amd import _lib      # (inside the tests, as in test_abi.py: not while the suite is being collected)
    return (_lib.lib.mm_bf_match_ratio_workspace_bytes(n_pairs, nq_cap, nt_cap),
            _lib.lib.mm_bf_workspace_bytes(n_pairs, nq_cap, nt_cap))


@pytest.mark.parametrize("variant", ["314"])
def test_fused_variants_hold_one_code_per_query_and_no_expanded_train_set(variant, monkeypatch):
    monkeypatch.setenv("MM_BF_VARIANT", variant)
    total, knn = sizes(499, 4000, 4000)
    assert knn == 256                                          # (never 0: the search wants a workspace pointer)
    assert total == knn + up(499 * 4000 * 4)
    # train sets the matrix-core kernels do not take (fewer than 64, 65536 and more): idx and dist behind the split buffers
    for nt_cap in (63, 65536):
        total, knn = sizes(9, 300, nt_cap)
        assert knn % 256 == 0 and total == knn + 2 * up(9 * 300 * 2 * 4)


@pytest.mark.parametrize("variant,per_train", [("114", 0)])
def test_other_variants_keep_idx_and_dist_behind_the_search_workspace(variant, per_train, monkeypatch):
    monkeypatch.setenv("MM_BF_VARIANT", variant)
    total, knn = sizes(9, 300, 300)
    assert knn > 0 and knn % 256 == 0
    assert total == knn + 2 * up(9 * 300 * 2 * 4)


@pytest.mark.parametrize("shape", [(499, 4000, 4000), (9, 300, 300), (9, 300, 63), (9, 300, 65536), (1, 70, 64)])
def test_a_removed_variant_sizes_as_the_default(shape, monkeypatch):
    """MM_BF_VARIANT=300 names a kernel that is gone: the compute calls refuse it (test_match_stage_gpu.py), the two size
    functions cannot fail and plan as if it were unset."""
    monkeypatch.delenv("MM_BF_VARIANT", raising=False)
    default = sizes(*shape)
    monkeypatch.setenv("MM_BF_VARIANT", "300")
    assert sizes(*shape) == default
    monkeypatch.setenv("MM_BF_VARIANT", "314")
    assert sizes(*shape) == default


@pytest.mark.parametrize("nt_cap,fused", [(63, False), (64, True), (65535, True), (65536, False)])
def test_layout_at_the_dispatch_boundaries(nt_cap, fused, monkeypatch):
    """One pair of 70 queries (the shape of test_dispatch_boundaries in test_match_stage_gpu.py), no environment: one code
    per query behind the search's workspace where the matrix-core kernel runs, idx + dist on either side of its range."""
    monkeypatch.delenv("MM_BF_VARIANT", raising=False)
    total, knn = sizes(1, 70, nt_cap)
    assert knn > 0 and knn % 256 == 0
    assert total == (knn + up(70 * 4) if fused else knn + 2 * up(70 * 8))
    if fused:
        assert knn == 256


def test_degenerate_shapes():
    for shape in ((0, 300, 300), (9, 0, 300), (9, 300, 0)):
        total, knn = sizes(*shape)
        assert total >= knn > 0 and total % 256 == 0
    assert sizes(9, 0, 300)[0] == sizes(9, 0, 300)[1]          # no queries: nothing behind the search's workspace
