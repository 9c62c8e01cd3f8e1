"""CPU: how mm_guided_match sizes its workspace (no compute calls)."""
import pytest


def up(x):
    return (x + 255) // 256 * 256


def size(n_pairs, cap):
    from meatmodeler_amd import _lib      # (inside the tests, as in test_abi.py: not while the suite is being collected)
    return _lib.lib.mm_guided_workspace_bytes(n_pairs, cap)


@pytest.mark.parametrize("shape", [(0, 320), (3, 0), (199, 4000)])
def test_workspace_is_positive_and_aligned(shape):
    assert size(*shape) > 0 and size(*shape) % 256 == 0      # (never 0: the call wants a workspace pointer)


def test_workspace_holds_its_tables():
    # per (pair, key point): five int32 tables, one pair of keys, two byte marks; per pair four counters
    rows = 199 * 4000
    assert size(199, 4000) >= 5 * up(4 * rows) + up(8 * rows) + 2 * up(rows) + up(16 * 199)
    assert size(199, 4000) <= 31 * rows + 16 * 199 + 10 * 256
    assert size(1, 320) <= size(2, 320) <= size(2, 321) and size(-1, 320) == size(0, 320) and size(3, -5) == size(3, 0)
