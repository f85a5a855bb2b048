"""CPU-only checks of the calls of the batched DenseSolver that act on a list of instances in place (include/piqp_amd.h: pq_solver_batch_solve_select,
pq_solver_batch_update_dense_select, pq_solver_batch_get_result_select_mem; piqp_amd.BatchDenseSolver.solve / update / result with instances=...), after
tests/test_batch_select_abi.py.  A pq_solver_batch cannot be set up without a device, so what can be asked here is what is refused before the handle is looked at -- a
NULL handle, a NULL list, count < 1, an unknown mem, order or field: any non-NULL value stands for the handle -- and what the Python wrapper refuses before it calls
the library.  The refusals that need a live handle (an entry out of range, an instance listed twice, a handle that was never set up, a result before any solve) are
in tests/test_dense_solver_batch_select_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

PQ_ERR_INVALID = -1
SENTINEL = 0x5A5A
IDX = np.array([0, 1], dtype=np.intc)
NEW = ("pq_solver_batch_solve_select", "pq_solver_batch_update_dense_select", "pq_solver_batch_get_result_select_mem")


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


def _calls(L, h, idx, count, mem=0, order=1, field=0):
    """the three _select calls with one handle, list and count; no value array is given (NULL = unchanged), the result goes to `o`"""
    o = np.full(4, -7.0)
    return {
        "pq_solver_batch_solve_select": lambda: L.pq_solver_batch_solve_select(h, idx, count),
        "pq_solver_batch_update_dense_select": lambda: L.pq_solver_batch_update_dense_select(h, idx, count, *[None] * 9, mem, order),
        "pq_solver_batch_get_result_select_mem": lambda: L.pq_solver_batch_get_result_select_mem(h, idx, count, field, o.ctypes.data, mem),
    }, o


def refused(L, rc, *words):
    assert rc == PQ_ERR_INVALID
    text = L.pq_last_error_string().decode()
    assert text != "" and all(w in text for w in words), text


def test_symbols_argtypes_and_header_lines(L):
    import piqp_amd
    vp, ci = C.c_void_p, C.c_int
    want = {
        "pq_solver_batch_solve_select": [vp, vp, ci],
        "pq_solver_batch_update_dense_select": [vp, vp, ci] + [vp] * 9 + [ci, ci],
        "pq_solver_batch_get_result_select_mem": [vp, vp, ci, ci, vp, ci],
    }
    assert sorted(want) == sorted(NEW)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "piqp_amd.h")).read()
    for name, argtypes in want.items():
        assert name in piqp_amd._lib.SYMBOLS
        fn = getattr(L, name)
        assert list(fn.argtypes) == argtypes, name
        assert fn.restype is C.c_int, name
        assert f"int {name}(pq_solver_batch *s, const int *idx, int count" in header, name
    # the contract stands in the header: listed, unlisted, the time rule, allocation, the refusals
    for words in ("A LISTED instance", "Of an UNLISTED instance no observable byte changes", "instance's OWN last update", "one device int buffer of `batch` entries",
                  "an instance listed twice"):
        assert words in header, words


@pytest.mark.parametrize("fn", NEW)
def test_a_null_handle_is_refused(L, fn):
    calls, o = _calls(L, None, IDX.ctypes.data, 2)
    refused(L, calls[fn](), fn, "null handle")
    assert o.tolist() == [-7.0] * 4


@pytest.mark.parametrize("fn", NEW)
def test_a_null_list_is_refused_with_its_own_text(L, fn):
    calls, o = _calls(L, C.c_void_p(SENTINEL), None, 2)
    refused(L, calls[fn](), fn, "idx is null")
    assert o.tolist() == [-7.0] * 4


@pytest.mark.parametrize("count", [0, -1, -3])
@pytest.mark.parametrize("fn", NEW)
def test_a_count_below_one_is_refused_with_its_value(L, fn, count):
    calls, o = _calls(L, C.c_void_p(SENTINEL), IDX.ctypes.data, count)
    refused(L, calls[fn](), fn, "count", str(count))
    assert o.tolist() == [-7.0] * 4


@pytest.mark.parametrize("mem", [2, -1])
@pytest.mark.parametrize("fn", NEW[1:])
def test_an_unknown_mem_is_refused_with_its_value(L, fn, mem):
    calls, o = _calls(L, C.c_void_p(SENTINEL), IDX.ctypes.data, 2, mem=mem)
    refused(L, calls[fn](), fn, "mem", str(mem))
    assert o.tolist() == [-7.0] * 4


@pytest.mark.parametrize("order", [2, -1])
def test_an_unknown_order_is_refused_with_its_value(L, order):
    calls, _ = _calls(L, C.c_void_p(SENTINEL), IDX.ctypes.data, 2, order=order)
    refused(L, calls["pq_solver_batch_update_dense_select"](), "pq_solver_batch_update_dense_select", "order", str(order))


@pytest.mark.parametrize("field", [10, -1])
def test_an_unknown_field_and_a_null_out_are_refused(L, field):
    calls, o = _calls(L, C.c_void_p(SENTINEL), IDX.ctypes.data, 2, field=field)
    refused(L, calls["pq_solver_batch_get_result_select_mem"](), "pq_solver_batch_get_result_select_mem", "field", str(field))
    assert o.tolist() == [-7.0] * 4
    refused(L, L.pq_solver_batch_get_result_select_mem(C.c_void_p(SENTINEL), IDX.ctypes.data, 2, 0, None, 0), "out")


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name}")


@pytest.fixture()
def stub():
    """a wrapper of batch 4, n = 3, p = 1, m = 2 whose every library call fails the test"""
    import piqp_amd
    k = piqp_amd.BatchDenseSolver.__new__(piqp_amd.BatchDenseSolver)
    k._owned = False
    k.L, k.h, k.device, k.kkt_solver, k.bounds = NoLibrary(), C.c_void_p(1), 0, 0, "shared"
    k.batch, k.n, k.p, k.m = 4, 3, 1, 2
    return k


def _wrappers(k):
    return {"solve": lambda inst: k.solve(instances=inst), "update": lambda inst: k.update(c=np.zeros((2, 3)), instances=inst),
            "result": lambda inst: k.result("x", instances=inst)}


def test_the_python_wrappers_refuse_a_bad_list_before_any_library_call(stub):
    """the lists of tests/test_batch_clone_abi.py::test_the_python_wrappers_refuse_a_bad_list_before_any_library_call: empty, not one-dimensional, not integers"""
    bad = ([], np.zeros((2, 2), dtype=np.intc), [[0, 1], [1, 0]], [0.5, 1.0], np.array([1.0]), ["a"], 3, [True, False], [[0], [1, 2]])
    for name, call in _wrappers(stub).items():
        for inst in bad:
            with pytest.raises(ValueError):
                call(inst)


def test_the_python_wrappers_refuse_an_instance_listed_twice_in_a_solve_or_an_update(stub):
    w = _wrappers(stub)
    for name in ("solve", "update"):
        for inst in ([1, 1], [0, 2, 0], np.array([3, 1, 2, 1])):
            with pytest.raises(ValueError, match="listed twice"):
                w[name](inst)
    # a result may repeat: the list passes, and the first thing after it is the library (the stub's AssertionError)
    with pytest.raises(AssertionError, match="library call"):
        w["result"]([1, 1])


def test_the_python_wrappers_check_the_stacks_against_the_length_of_the_list(stub):
    k = stub
    shapes = dict(P=(3, 3), c=(3,), A=(1, 3), b=(1,), G=(2, 3), h_l=(2,), h_u=(2,), x_l=(3,), x_u=(3,))
    for name, tail in shapes.items():
        for lead in (4, 3, 1):  # the batch, and two other lengths that are not the list's
            with pytest.raises(ValueError, match=name):
                k.update(instances=[2, 0], **{name: np.zeros((lead,) + tail)})
        with pytest.raises(ValueError, match=name):
            k.update(instances=[2, 0], **{name: np.zeros((2,) + tail + (1,))})
        # the right shape passes the checks: the next thing is the library
        with pytest.raises(AssertionError, match="library call pq_solver_batch_update_dense_select"):
            k.update(instances=[2, 0], **{name: np.zeros((2,) + tail)})
    # without a list the stacks are the whole batch's, as before
    with pytest.raises(ValueError, match="c"):
        k.update(c=np.zeros((2, 3)))
    with pytest.raises(AssertionError, match="library call pq_solver_batch_update_dense"):
        k.update(c=np.zeros((4, 3)))
