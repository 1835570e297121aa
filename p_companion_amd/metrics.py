"""Metrics on the device -- drop-in for src/utils/metrics.py (Metrics.evaluate_model runs every
epoch in train.train and selects the best checkpoint, train.py:55-70).

The similarity product [B*K,128] x [128,B] is the shared NT GEMM (pc_linear_forward: fp32 MFMA for few rows, fp32-grade
six-product bf16 MFMA for many), hit@k is a rank kernel
(one wave per row), relevance a cosine kernel; only the final scalar means are read back.
Reproduces the reference's quirk: ground truth is arange(B*K) against B columns, so rows >= B can
never hit (metrics.py:95-100).

Over a ComplementaryIndexLoader whose arrays live on the model's GPU the whole evaluation is one foreign call
(pc_joint_eval_epoch, csrc/evaluate.hip): the top-K and the type projections once per TYPE, the hit counts from a B x B x D
product whose epilogue compares and counts (no score matrix), the five metrics formed on the device and read back once.

Metrics.catalogue_metrics is not in the reference: it turns the ranks of held-out complements among ALL products of their
type (PCompanionInference.rank_targets -> pc_rank_grouped) into hit@k / MRR / median rank -- what the served lists are
worth, which the in-batch proxy above cannot say."""
from typing import Dict

import numpy as np
import torch

from . import ops


class Metrics:
    @staticmethod
    def hit_at_k(predictions: torch.Tensor, ground_truth: torch.Tensor, k: int) -> float:
        """predictions [R, C] scores; ground_truth [R]; metrics.py:7-27.  The device kernel covers
        the only use in the reference (ground_truth == arange(R))."""
        k = min(k, predictions.size(1))
        if not torch.equal(ground_truth.cpu(), torch.arange(predictions.size(0))):
            raise NotImplementedError("hit_at_k kernel: ground_truth must be arange(rows) (metrics.py:100)")
        rank = ops.hit_rank(predictions.contiguous().float())
        return float((rank < k).float().mean())

    @staticmethod
    def type_diversity(predicted_types: torch.Tensor) -> float:
        """metrics.py:29-42: unique COLUMNS of [B,K] / K (tiny integer matrix: host side)."""
        if predicted_types.numel() == 0:
            return 0.0
        cols = np.unique(predicted_types.cpu().numpy(), axis=1)
        return cols.shape[1] / predicted_types.size(1)

    @staticmethod
    def mean_relevance(predictions: torch.Tensor, ground_truth: torch.Tensor) -> float:
        """metrics.py:44-60"""
        return float(ops.cosine_rows(predictions.contiguous().float(), ground_truth.contiguous().float()).mean())

    @staticmethod
    def catalogue_metrics(slot: torch.Tensor, rank: torch.Tensor, ks=(1, 3, 10, 100), take: torch.Tensor = None) -> Dict[str, float]:
        """slot / rank [N] int32 as PCompanionInference.rank_targets returns them (slot -1: no predicted type is the
        target's; rank: the target's position among all products of its type, -1 where there is none); take [N] bool:
        the pairs that count (None: all).  Returns
          pairs        the number of pairs that count
          type_hit     the share of them with slot >= 0
          hit@k        the share of ALL of them with 0 <= rank < k  (k <= 16: the target is in recommend_batch(query, k)'s lists)
          mrr          the mean of 1 / (rank + 1), 0 for a pair without a rank
          median_rank  the median rank over the pairs that have one (the mean of the two middle ranks for an even number;
                       -1.0 when no pair has one)
        Integer counts and one float64 sum over the [N] vector in torch's fixed reduction order, formed where the tensors
        live; ONE read-back.  ValueError if no pair counts."""
        ks = tuple(int(k) for k in ks)
        if slot.shape != rank.shape or slot.dim() != 1 or any(k < 1 for k in ks):
            raise ValueError("catalogue_metrics: slot and rank must be [N] and every k >= 1")
        take = torch.ones_like(slot, dtype=torch.bool) if take is None else take.bool()
        ranked = take & (rank >= 0)
        counts = [take.sum(), (take & (slot >= 0)).sum(), ranked.sum()] + [(ranked & (rank < k)).sum() for k in ks]
        rr = torch.where(ranked, 1.0 / (rank.double() + 1.0), torch.zeros((), dtype=torch.float64, device=rank.device)).sum()
        # the two middle ranks: unranked pairs sort to the end
        ordered = torch.where(ranked, rank, torch.full_like(rank, torch.iinfo(torch.int32).max)).sort().values
        m = counts[2]
        mid = torch.stack([(m - 1).clamp(min=0) // 2, m // 2]).clamp(max=max(rank.numel() - 1, 0))
        middle = ordered[mid] if rank.numel() else torch.zeros(2, dtype=torch.int32, device=rank.device)
        out = torch.cat([torch.stack(counts).double(), rr.reshape(1), middle.double()]).cpu().tolist()      # the ONE read-back
        pairs, typed, n_ranked = (int(x) for x in out[:3])
        if pairs == 0:
            raise ValueError("catalogue_metrics: no pair to evaluate (an empty set of +1 pairs)")
        res = {"pairs": pairs, "type_hit": typed / pairs}
        for k, h in zip(ks, out[3:3 + len(ks)]):
            res[f"hit@{k}"] = int(h) / pairs
        res["mrr"] = out[3 + len(ks)] / pairs
        res["median_rank"] = 0.5 * (out[-2] + out[-1]) if n_ranked else -1.0
        return res

    @staticmethod
    def intra_list_similarity(idx: torch.Tensor, table: torch.Tensor, scale: torch.Tensor = None, chunk: int = 4096) -> torch.Tensor:
        """How alike the products inside a served list are: idx [..., n] product ids (-1: none) as recommend_batch /
        recommend_diverse_batch / ops.diversify_lists return them, table [P, D], scale [P] or None -> the mean over the lists with
        at least two products of the list's mean pairwise similarity <table[a], table[b]> scale[a] scale[b] over its distinct
        pairs (scale = ops.inv_norm(table): the cosine).  A 0-dim float64 tensor where the tensors live (0 when no list holds
        two products); nothing is read back.  Plain torch in float64, `chunk` lists at a time: a reporting figure, not a
        serving path."""
        idx = idx.reshape(-1, idx.shape[-1]).long()
        total = torch.zeros((), dtype=torch.float64, device=table.device)
        lists = torch.zeros((), dtype=torch.float64, device=table.device)
        for lo in range(0, idx.shape[0], int(chunk)):
            ids = idx[lo:lo + int(chunk)]
            live = ids >= 0
            rows = table[ids.clamp(min=0)].double()
            if scale is not None:
                rows = rows * scale[ids.clamp(min=0)].double()[..., None]
            rows = rows * live[..., None]
            gram = rows @ rows.transpose(1, 2)                                  # [lists, n, n]
            pair_sum = (gram.sum((1, 2)) - gram.diagonal(dim1=1, dim2=2).sum(1)) / 2
            k = live.sum(1).double()
            pairs = k * (k - 1) / 2
            has = pairs > 0
            total += torch.where(has, pair_sum / pairs.clamp(min=1), torch.zeros_like(pair_sum)).sum()
            lists += has.sum()
        return total / lists.clamp(min=1)

    @staticmethod
    def _fused_refusal(model, data_loader):
        """Why the one-call evaluation (pc_joint_eval_epoch) does not serve (model, data_loader); None: it does."""
        from .data import ComplementaryIndexLoader
        from .p_companion import PCompanion
        if not isinstance(data_loader, ComplementaryIndexLoader):
            return "the loader is not a ComplementaryIndexLoader"
        if not isinstance(model, PCompanion):
            return "the model is not a PCompanion"
        feats, table = data_loader.features, model.product_embeddings.weight
        if not (torch.is_tensor(feats) and feats.is_cuda and table.is_cuda and feats.device == table.device):
            return "the loader's arrays and the model are not on the same GPU"
        if tuple(feats.shape) != tuple(table.shape) or data_loader.type_idx.dtype != torch.int32:
            return "the loader's feature table and the model's product table differ in shape"
        pairs = data_loader.dataset.pairs
        if torch.is_tensor(pairs) and pairs.device != table.device:
            return "the dataset's pairs live on another device"
        n, b = len(data_loader.dataset), data_loader.batch_size
        if n == 0 or b < 10 or 0 < n % b < 10:
            return "an empty split, or a batch of fewer than 10 rows (the existing loop reproduces metrics.py:103 there)"
        if not 1 <= int(model.config.NUM_COMP_TYPES) <= min(8, model.query_type_embeddings.weight.shape[0]):
            return "NUM_COMP_TYPES outside 1..8"
        return None

    @staticmethod
    def evaluate_on_device(model, loader) -> Dict[str, torch.Tensor]:
        """metrics.py:62-117 as one foreign call with NOTHING read back: ops.joint_eval_epoch's dict of device tensors
        ("metrics" double[5] in the order hit@1, hit@3, hit@10, type_diversity, mean_relevance; per-batch "stats" / "cos_sum";
        the plan's "topk_table").  Leaves the loader as iterating it would: epoch + 1, step + number of batches."""
        why = Metrics._fused_refusal(model, loader)
        if why is not None:
            raise ValueError("evaluate_on_device: " + why)
        model.eval()
        params = model._tensor_dict()
        params["product_embeddings.weight"] = model.product_embeddings.weight
        pairs = loader.epoch_pairs()                       # (advances loader.epoch; the loop's shuffled order)
        source = (loader.features, loader.type_idx, int(loader.dataset.bpg.n_types), int(loader.seed))
        with torch.no_grad():
            out = ops.joint_eval_epoch(params, pairs.contiguous(), source, loader.step, loader.batch_size,
                                       int(model.config.NUM_COMP_TYPES), bad=model._bad_counter())
        loader.step += len(loader)
        return out

    @staticmethod
    def evaluate_model(model: torch.nn.Module, data_loader, device, fused=None) -> Dict[str, float]:
        """metrics.py:62-117.  fused=None: over a ComplementaryIndexLoader whose arrays live on the model's GPU the whole
        evaluation is ONE foreign call (pc_joint_eval_epoch: the batches are never built, no [B*K, B] score matrix, one
        read-back of the five metrics); any other loader -- and a last batch of 1..9 rows -- takes the loop below.
        fused=False forces the loop; fused=True raises ValueError where the one-call form does not apply."""
        if fused is None or fused:
            why = Metrics._fused_refusal(model, data_loader)
            if why is None:
                m = Metrics.evaluate_on_device(model, data_loader)["metrics"].cpu().tolist()      # the ONE read-back
                return dict(zip(("hit@1", "hit@3", "hit@10", "type_diversity", "mean_relevance"), m))
            if fused:
                raise ValueError("evaluate_model(fused=True): " + why)
        model.eval()
        metrics = {"hit@1": 0.0, "hit@3": 0.0, "hit@10": 0.0, "type_diversity": 0.0, "mean_relevance": 0.0}
        num_batches = 0
        with torch.no_grad():
            for batch in data_loader:
                batch = {k: v.to(device) if torch.is_tensor(v) else v for k, v in batch.items()}
                outputs = model(batch)
                proj = outputs["projected_embeddings"]
                targets = batch["target_features"].float().contiguous()
                similarities = ops.linear_forward(proj.reshape(-1, proj.size(-1)).contiguous(), targets)   # [B*K, B]
                rank = ops.hit_rank(similarities)
                for k in [1, 3, min(10, similarities.size(1))]:
                    metrics[f"hit@{k}"] += float((rank < min(k, similarities.size(1))).float().mean())
                metrics["type_diversity"] += Metrics.type_diversity(outputs["complementary_types"])
                metrics["mean_relevance"] += Metrics.mean_relevance(proj, batch["positive_items"].to(device))
                num_batches += 1
        for key in metrics:
            metrics[key] /= max(num_batches, 1)
        return metrics
