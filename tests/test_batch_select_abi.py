"""CPU-only checks of the calls of the batched sparse solver that act on a list of instances in place (include/piqp_amd.h: pq_batch_solve_select,
pq_batch_update_select_mem, pq_batch_update_data_select_mem, pq_batch_get_result_select_mem, pq_batch_arena_row; piqp_amd.BatchSparseSolver.solve / update /
update_data / result with instances=...).  A pq_batch cannot exist without a device (pq_batch_create refuses), so what can be asked here is what is refused before
the handle is looked at -- a NULL handle, a NULL list, count < 1, an unknown mem or field: any non-NULL value stands for the handle -- and what the Python wrapper
refuses before it calls the library.  The refusals that need a live handle (an entry out of range, an instance listed twice, a handle that was never set up) are in
tests/test_batch_select_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

PQ_ERR_INVALID = -1
SENTINEL = 0x5A5A
IDX = np.array([0, 1], dtype=np.intc)
NEW = ("pq_batch_solve_select", "pq_batch_update_select_mem", "pq_batch_update_data_select_mem", "pq_batch_get_result_select_mem", "pq_batch_arena_row")


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


def _calls(L, h, idx, count, mem=0, field=0, out=None):
    """the four _select calls with one handle, list and count; no value array is given (NULL = unchanged), the result goes to `out`"""
    o = np.full(4, -7.0) if out is None else out
    return {
        "pq_batch_solve_select": lambda: L.pq_batch_solve_select(h, idx, count),
        "pq_batch_update_select_mem": lambda: L.pq_batch_update_select_mem(h, idx, count, *[None] * 6, mem),
        "pq_batch_update_data_select_mem": lambda: L.pq_batch_update_data_select_mem(h, idx, count, *[None] * 9, mem),
        "pq_batch_get_result_select_mem": lambda: L.pq_batch_get_result_select_mem(h, idx, count, field, o.ctypes.data, mem),
    }, o


def refused(L, rc, *words):
    assert rc == PQ_ERR_INVALID
    text = L.pq_last_error_string().decode()
    assert text != "" and all(w in text for w in words), text


def test_symbols_and_argtypes(L):
    import piqp_amd
    vp, ci = C.c_void_p, C.c_int
    want = {
        "pq_batch_solve_select": [vp, vp, ci],
        "pq_batch_update_select_mem": [vp, vp, ci] + [vp] * 6 + [ci],
        "pq_batch_update_data_select_mem": [vp, vp, ci] + [vp] * 9 + [ci],
        "pq_batch_get_result_select_mem": [vp, vp, ci, ci, vp, ci],
        "pq_batch_arena_row": [vp, ci, vp],
    }
    assert sorted(want) == sorted(NEW)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "piqp_amd.h")).read()
    for name, argtypes in want.items():
        assert name in piqp_amd._lib.SYMBOLS
        fn = getattr(L, name)
        assert list(fn.argtypes) == argtypes, name
        assert fn.restype is C.c_int, name
        assert f"int {name}(" in header, name


@pytest.mark.parametrize("fn", NEW[:4])
def test_a_null_handle_is_refused(L, fn):
    calls, o = _calls(L, None, IDX.ctypes.data, 2)
    refused(L, calls[fn](), fn, "null handle")
    assert o.tolist() == [-7.0] * 4


@pytest.mark.parametrize("fn", NEW[:4])
def test_a_null_list_is_refused_with_its_own_text(L, fn):
    calls, o = _calls(L, C.c_void_p(SENTINEL), None, 2)
    refused(L, calls[fn](), fn, "idx is null")
    assert o.tolist() == [-7.0] * 4


@pytest.mark.parametrize("count", [0, -1, -3])
@pytest.mark.parametrize("fn", NEW[:4])
def test_a_count_below_one_is_refused_with_its_value(L, fn, count):
    calls, o = _calls(L, C.c_void_p(SENTINEL), IDX.ctypes.data, count)
    refused(L, calls[fn](), fn, "count", str(count))
    assert o.tolist() == [-7.0] * 4


@pytest.mark.parametrize("mem", [2, -1])
@pytest.mark.parametrize("fn", NEW[1:4])
def test_an_unknown_mem_is_refused_with_its_value(L, fn, mem):
    calls, o = _calls(L, C.c_void_p(SENTINEL), IDX.ctypes.data, 2, mem=mem)
    refused(L, calls[fn](), fn, "mem", str(mem))
    assert o.tolist() == [-7.0] * 4


@pytest.mark.parametrize("field", [10, -1])
def test_an_unknown_field_and_a_null_out_are_refused(L, field):
    calls, o = _calls(L, C.c_void_p(SENTINEL), IDX.ctypes.data, 2, field=field)
    refused(L, calls["pq_batch_get_result_select_mem"](), "pq_batch_get_result_select_mem", "field", str(field))
    assert o.tolist() == [-7.0] * 4
    refused(L, L.pq_batch_get_result_select_mem(C.c_void_p(SENTINEL), IDX.ctypes.data, 2, 0, None, 0), "out")


def test_arena_row_of_a_null_handle_or_into_a_null_out_is_refused(L):
    o = np.full(4, -7.0)
    refused(L, L.pq_batch_arena_row(None, 0, o.ctypes.data), "pq_batch_arena_row")
    refused(L, L.pq_batch_arena_row(C.c_void_p(SENTINEL), 0, None), "pq_batch_arena_row")
    assert o.tolist() == [-7.0] * 4


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name}")


@pytest.fixture()
def stub():
    """a wrapper of batch 4, n = 3, p = 1, m = 2 whose every library call fails the test"""
    import piqp_amd
    k = piqp_amd.BatchSparseSolver.__new__(piqp_amd.BatchSparseSolver)
    k._owned = False
    k.L, k.h, k.device, k.bounds = NoLibrary(), C.c_void_p(1), 0, "shared"
    k.batch, k.n, k.p, k.m, k._nnz = 4, 3, 1, 2, (3, 3, 2)
    return k


def _wrappers(k):
    return {"solve": lambda inst: k.solve(instances=inst), "update": lambda inst: k.update(c=np.zeros((2, 3)), instances=inst),
            "update_data": lambda inst: k.update_data(P_values=np.zeros((2, 3)), instances=inst), "result": lambda inst: k.result("x", instances=inst),
            "result_device": lambda inst: k.result("x", device=True, instances=inst)}


def test_the_python_wrappers_refuse_a_bad_list_before_any_library_call(stub):
    """the lists of tests/test_batch_clone_abi.py::test_the_python_wrappers_refuse_a_bad_list_before_any_library_call"""
    bad = ([], np.zeros((2, 2), dtype=np.intc), [[0, 1], [1, 0]], [0.5, 1.0], np.array([1.0]), ["a"], 3, [True, False], [[0], [1, 2]])
    for name, call in _wrappers(stub).items():
        for inst in bad:
            with pytest.raises(ValueError):
                call(inst)


def test_the_python_wrappers_refuse_an_instance_listed_twice_in_a_solve_or_an_update(stub):
    w = _wrappers(stub)
    for name in ("solve", "update", "update_data"):
        for inst in ([1, 1], [0, 2, 0], np.array([3, 1, 2, 1])):
            with pytest.raises(ValueError, match="listed twice"):
                w[name](inst)
    # a result may repeat: the list passes, and the first thing after it is the library (the stub's AssertionError)
    with pytest.raises(AssertionError, match="library call"):
        w["result"]([1, 1])


def test_the_python_wrappers_check_the_stacks_against_the_length_of_the_list(stub):
    k = stub
    lens = dict(c=3, b=1, h_l=2, h_u=2, x_l=3, x_u=3)
    for name, ln in lens.items():
        for shape in ((4, ln), (3, ln), (2, ln + 1), (ln,), (2, ln, 1)):
            with pytest.raises(ValueError, match=name):
                k.update(instances=[2, 0], **{name: np.zeros(shape)})
            with pytest.raises(ValueError, match=name):
                k.update_data(instances=[2, 0], **{name: np.zeros(shape)})
        # the right shape passes the checks: the next thing is the library
        with pytest.raises(AssertionError, match="library call pq_batch_update_select_mem"):
            k.update(instances=[2, 0], **{name: np.zeros((2, ln))})
    for name, ln in dict(P_values=3, A_values=3, G_values=2).items():
        for shape in ((4, ln), (2, ln + 1), (ln,)):
            with pytest.raises(ValueError, match=name):
                k.update_data(instances=[2, 0], **{name: np.zeros(shape)})
        with pytest.raises(AssertionError, match="library call pq_batch_update_data_select_mem"):
            k.update_data(instances=[2, 0], **{name: np.zeros((2, ln))})
    # without a list the stacks are the whole batch's, as before
    with pytest.raises(AssertionError):
        k.update(c=np.zeros((2, 3)))
