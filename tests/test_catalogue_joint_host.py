"""Host side of joint training over a device-resident catalogue, without a GPU: the two new entries are declared and bind,
their wrappers refuse CPU tensors, and ComplementaryIndexDataset's refusals of a DeviceBPG happen before anything reaches
a kernel (here a DeviceBPG over CPU tensors)."""
import pytest
import torch

from test_abi import header_functions


def test_new_entries_are_declared_and_bind():
    from p_companion_amd import _lib
    fns = header_functions()
    for name in ("pc_comp_split_pairs", "pc_build_complementary_batch_dim"):
        assert name in fns and name in _lib.SIGNATURES
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name][1]


def test_wrappers_refuse_cpu_tensors():
    from p_companion_amd import ops
    comp, sim = torch.zeros(4, 2, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.comp_split_pairs(comp, sim, 0, "train")
    pairs = torch.zeros(2, 3, dtype=torch.int32)
    for d in (128, 256):
        with pytest.raises(TypeError):
            ops.build_complementary_batch(pairs, torch.zeros(5, d), torch.zeros(5, dtype=torch.int32), 4, 0, 0)


def test_split_bounds_are_the_host_rule():
    from p_companion_amd import ops
    for n in (1, 7, 10, 101, 999_983):
        lo_v, hi_v = ops.split_bounds(n, "val")
        assert ops.split_bounds(n, "train") == (0, int(0.8 * n)) and (lo_v, hi_v) == (int(0.8 * n), int(0.9 * n))
        assert ops.split_bounds(n, "test") == (int(0.9 * n), n)


def _cpu_device_bpg(**over):
    from p_companion_amd.data import DeviceBPG
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    arrays = {"n_products": 10, "max_degree": 2, "type_idx": i32(10), "cv_rowptr": i32(11), "cv_col": i32(0),
              "sim_pairs": i32(3, 2), "sim_rowptr": i32(11), "sim_col": i32(3), "comp_pairs": i32(4, 2),
              "features": torch.zeros(10, 128)}
    drop = over.pop("drop", ())
    for k in drop:
        del arrays[k]
    return DeviceBPG(arrays, n_types=5, dim=128, **over)


def test_device_dataset_refusals():
    from p_companion_amd.data import ComplementaryIndexDataset
    with pytest.raises(ValueError, match="philox"):
        ComplementaryIndexDataset(_cpu_device_bpg(), "train", sampler="cpython")
    with pytest.raises(ValueError, match="world = 1"):
        ComplementaryIndexDataset(_cpu_device_bpg(rank=1, world=2), "train")
    with pytest.raises(ValueError, match="complementary pairs"):
        ComplementaryIndexDataset(_cpu_device_bpg(drop=("comp_pairs",)), "train")
    with pytest.raises(ValueError, match="features"):
        ComplementaryIndexDataset(_cpu_device_bpg(drop=("features",)), "val")
    with pytest.raises(ValueError, match="mode"):
        ComplementaryIndexDataset(_cpu_device_bpg(), "holdout")
    with pytest.raises(TypeError):                          # CPU arrays reach the wrapper, which refuses them
        ComplementaryIndexDataset(_cpu_device_bpg(), "train")


def test_error_codes_before_any_launch():
    """The argument checks of both entries return before anything touches a device."""
    import ctypes
    from p_companion_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    split = lambda comp, nc, sim, ns, lo, hi, mode, out=p: L.pc_comp_split_pairs(comp, nc, sim, ns, lo, hi, 0, mode, out, None)
    assert split(p, 4, p, 6, 3, 3, 0) == 0                           # an empty range: nothing to do
    for args in ((p, 4, p, 6, 0, 8, 0, None),                          # null out
                 (None, 4, p, 6, 0, 8, 0), (p, 4, None, 6, 0, 8, 0),   # null pairs with a count
                 (None, 0, None, 0, 0, 0, 0),                         # n = 0
                 (p, 1 << 31, p, 0, 0, 1, 0), (p, 1 << 30, p, 1 << 30, 0, 1, 0),   # n >= 2^31
                 (p, -1, p, 6, 0, 1, 0),
                 (p, 4, p, 6, -1, 8, 0), (p, 4, p, 6, 5, 4, 0), (p, 4, p, 6, 0, 11, 0),   # 0 <= lo <= hi <= n
                 (p, 4, p, 6, 0, 8, 3), (p, 4, p, 6, 0, 8, -1)):      # mode outside 0..2
        assert split(*args) == -1, args
    build = lambda dim, batch=4, feats=p: L.pc_build_complementary_batch_dim(p, batch, feats, p, 5, dim, 0, 0, p, p, p, p, p, p,
                                                                             None, None)
    for dim in (0, 64, 192, 512):
        assert build(dim) == -2, dim
    assert build(128, feats=None) == -1 and build(256, batch=0) == -1
