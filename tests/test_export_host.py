"""Host side of the device-CSR embedding export: the Mapping a DeviceBPG export returns, and the refusals that happen
before anything reaches a kernel.  No GPU needed."""
from collections.abc import Mapping
from types import SimpleNamespace

import pytest
import torch


def cfg():
    return SimpleNamespace(PRODUCT_EMB_DIM=128, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                           MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=100, DEVICE=torch.device("cpu"),
                           LEARNING_RATE=1e-3)


def test_embedding_mapping_reads_rows_by_product_id():
    from p_companion_amd.data import EmbeddingMapping
    t = torch.arange(12 * 4, dtype=torch.float32).reshape(12, 4)
    m = EmbeddingMapping(t)
    assert isinstance(m, Mapping) and not isinstance(m, dict)
    assert len(m) == 12 and list(m) == [f"P{i:06d}" for i in range(12)]
    assert torch.equal(m["P000007"], t[7]) and m.get("P000012") is None
    assert "P000011" in m and "P000012" not in m and "P11" not in m and "Q000001" not in m and 3 not in m
    with pytest.raises(KeyError):
        m["P-00001"]
    with pytest.raises(TypeError):
        m["P000001"] = t[0]                          # read-only
    big = EmbeddingMapping(torch.zeros(1_234_567, 1))
    assert "P1234566" in big and list(big.keys())[1_000_000] == "P1000000"
    with pytest.raises(TypeError):
        EmbeddingMapping(torch.zeros(3))


def test_sharded_device_bpg_is_refused():
    from p_companion_amd.data import DeviceBPG
    from p_companion_amd.product2vec import Product2Vec
    bpg = DeviceBPG({"n_products": 10, "max_degree": 2}, n_types=5, dim=128, rank=1, world=2)
    with pytest.raises(ValueError, match="world = 1"):
        Product2Vec(cfg()).generate_all_embeddings(bpg)


def test_export_refuses_host_tensors():
    from p_companion_amd import ops
    from p_companion_amd.product2vec import Product2Vec
    model = Product2Vec(cfg()).eval()
    rowptr, col = torch.tensor([0, 1, 1], dtype=torch.int32), torch.tensor([1], dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.export_embeddings(model._tensor_dict(), torch.zeros(2, 128), rowptr, col)
    with pytest.raises(TypeError):
        model.generate_embedding_table(torch.zeros(2, 128), rowptr, col)
