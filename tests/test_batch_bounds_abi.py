"""CPU-only checks of pq_batch_set_bound_sets and of BatchSparseSolver(bounds=...): the refusals that come before a handle or a device is needed.  What needs a
handle (pq_batch_create wants a device) is in tests/test_batch_bounds_gpu.py."""
import pytest

PQ_ERR_INVALID = -1


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


def test_null_handle_is_refused_whatever_the_mode(L):
    for mode in (0, 1, 2, -1, 7):
        assert L.pq_batch_set_bound_sets(None, mode) == PQ_ERR_INVALID and L.pq_last_error_string().decode()


def test_bound_lists_hook_refuses_null_arguments(L):
    import numpy as np
    counts = np.zeros(4, dtype=np.int32)
    assert L.pq_batch_bound_lists(None, 0, counts.ctypes.data, None, None, None, None, None) == PQ_ERR_INVALID and L.pq_last_error_string().decode()


def test_python_refuses_a_bad_bounds_string_before_any_library_call(monkeypatch):
    import piqp_amd
    from piqp_amd import _lib

    def no_call():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_call)
    for bad in ("x", "", "SHARED", "per-instance", None, 1):
        with pytest.raises(ValueError, match="bounds"):
            piqp_amd.BatchSparseSolver(bounds=bad)
