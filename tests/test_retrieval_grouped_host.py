"""pc_retrieve_topk_grouped's host side, without a GPU: the workspace query depends on rows, n_types, n and slices only
(partial lists of rows x slices x n entries dominate it) and the Python wrappers refuse CPU tensors."""
import pytest
import torch


def test_workspace_bytes_depend_on_the_plan_only():
    from p_companion_amd import _lib
    L = _lib.lib()
    ws = L.pc_retrieve_topk_grouped_workspace_bytes
    rows, types = 12288, 100
    full = ws(rows, types, 16, 16)
    partials = rows * 16 * 16 * 8
    assert partials <= full < partials + 8 * (rows + types) * 4 + 8 * 256
    assert ws(rows, types, 16, 0) == full                               # 0 = automatic = 16 slices
    assert ws(rows, types, 16, 1) < ws(rows, types, 16, 7) < full < ws(rows, types, 16, 64)
    assert ws(rows, 34_800, 10, 0) > ws(rows, 100, 10, 0)
    for bad in ((0, types, 10, 0), (rows, 0, 10, 0), (rows, types, 0, 0), (rows, types, 17, 0), (rows, types, 10, -1),
                (rows, types, 10, 65)):
        assert ws(*bad) == 0, bad


def test_wrappers_refuse_cpu_tensors():
    from p_companion_amd import ops
    proj = torch.zeros(2, 128)
    types = torch.zeros(2, dtype=torch.int32)
    rowptr = torch.tensor([0, 1], dtype=torch.int32)
    col = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.retrieve_topk_grouped(proj, types, rowptr, col, torch.zeros(1, 128), 5)
    with pytest.raises(TypeError):
        ops.type_csr(types, 1)
