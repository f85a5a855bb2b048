"""Problem data in GPU memory, the part that needs no GPU: how the binding picks the storage order it reports to pq_solver_*_mem and what it refuses
before the library is called (piqp_amd/kkt.py: tensor_layout, check_device_tensor, device_call)."""
import numpy as np
import pytest
import torch

from piqp_amd import kkt


def test_layout_of_a_contiguous_tensor_is_row_major():
    t = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    out, layout = kkt.tensor_layout(t)
    assert layout == kkt.ROW_MAJOR and out is t


def test_layout_of_a_transposed_view_is_col_major():
    base = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    t = base.t()  # 3 x 4, stored column by column
    assert not t.is_contiguous()
    out, layout = kkt.tensor_layout(t)
    assert layout == kkt.COL_MAJOR and out is t
    assert out.data_ptr() == base.data_ptr()


def test_layout_of_a_sliced_view_is_made_contiguous():
    base = torch.arange(40, dtype=torch.float64).reshape(5, 8)
    t = base[1:4, ::2]
    assert not t.is_contiguous() and not t.t().is_contiguous()
    out, layout = kkt.tensor_layout(t)
    assert layout == kkt.ROW_MAJOR and out.is_contiguous()
    assert torch.equal(out, t) and out.data_ptr() != base.data_ptr()


def test_layout_of_degenerate_shapes():
    # a 1 x n tensor is contiguous in both senses: the plain-copy case wins
    assert kkt.tensor_layout(torch.zeros(1, 7, dtype=torch.float64))[1] == kkt.ROW_MAJOR
    assert kkt.tensor_layout(torch.zeros(7, 1, dtype=torch.float64))[1] == kkt.ROW_MAJOR


def test_enum_values_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "piqp_amd.h")).read()
    m = re.search(r"enum\s*\{\s*PQ_COL_MAJOR\s*=\s*(\d+)\s*,\s*PQ_ROW_MAJOR\s*=\s*(\d+)\s*\}", txt)
    assert m and (int(m.group(1)), int(m.group(2))) == (kkt.COL_MAJOR, kkt.ROW_MAJOR)
    m = re.search(r"PQ_MEM_HOST\s*=\s*(\d+)\s*,\s*PQ_MEM_DEVICE\s*=\s*(\d+)", txt)
    assert m and (int(m.group(1)), int(m.group(2))) == (kkt.MEM_HOST, kkt.MEM_DEVICE)


def test_numpy_and_cpu_tensors_do_not_select_the_device_path():
    assert not kkt.device_call((np.eye(3), None, np.zeros(3)))
    assert not kkt.device_call((torch.eye(3, dtype=torch.float64), None))
    assert not kkt.device_call(())


def test_float32_is_refused():
    with pytest.raises(TypeError, match="float64"):
        kkt.check_device_tensor("P", torch.eye(3, dtype=torch.float32), (3, 3), 0)


def test_shape_mismatch_is_refused():
    with pytest.raises(ValueError, match="shape"):
        kkt.check_device_tensor("A", torch.zeros(2, 4, dtype=torch.float64), (2, 3), 0)
    with pytest.raises(ValueError, match="shape"):
        kkt.check_device_tensor("c", torch.zeros(3, 1, dtype=torch.float64), (3,), 0)


def test_cpu_tensor_where_device_memory_is_meant_is_refused():
    # a device-mode call hands raw addresses to kernels: a CPU tensor's address means nothing there
    with pytest.raises(TypeError, match="CPU torch tensor"):
        kkt.check_device_tensor("G", torch.zeros(2, 3, dtype=torch.float64), (2, 3), 0)
    with pytest.raises(TypeError, match="CPU torch tensor"):
        kkt.to_device_args(dict(P=torch.eye(3, dtype=torch.float64), c=None), dict(P=(3, 3), c=(3,)), 0, matrices=("P",))


def test_numpy_argument_of_the_wrong_shape_is_refused_before_any_copy():
    with pytest.raises(ValueError, match="shape"):
        kkt.to_device_args(dict(c=np.zeros(4)), dict(c=(3,)), 0)
