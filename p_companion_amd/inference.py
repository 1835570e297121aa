"""Serving counterpart of the reference's inference.py:10-124 (PCompanionInference).

The reference file is a non-running stub (it builds PCompanion without its embeddings argument and
feeds forward() keys it does not read), so the semantics are taken from its recommend() body
(:64-124): run the model on the query, then for every predicted complementary type take the products
of that type, score them by <projected embedding, product features> and keep torch.topk of the scores.
Here the candidate search of all (query, type) rows is one launch of pc_retrieve_topk over a
type-grouped CSR of the product table.  Over a DeviceBPG (a 10 M / 100 M catalogue generated in HBM) the CSR is
built on the device (ops.type_csr) and the search is pc_retrieve_topk_grouped, which scores each type's candidates
as a tiled fp32 GEMM; neither type_idx nor the features are copied to the host.

rank_targets / evaluate_catalogue are not in the reference: they say where a KNOWN complement stands in what recommend_batch
serves -- its rank among all products of its type (pc_rank_grouped: the grouped retrieval's schedule and score bits, the
selection replaced by a count) -- and fold the held-out "test" pairs into hit@k / MRR / median rank.
set_exclusions / set_eligible keep the query, its co-viewed substitutes and unservable products out of both
(pc_retrieve_topk_grouped_excluding / pc_rank_grouped_excluding).
catalogue= serves the lists of up to 16 from a bf16 copy of the product table (pc_retrieve_topk_grouped_bf16): half the bytes,
scored against the unrounded query; the scores are those of the ROUNDED table.
recommend_diverse_batch re-ranks recommend_batch's long list for diversity inside a type, on the device: a greedy maximal-
marginal-relevance pick of the products to show (pc_diversify_lists over the fp32 features, pc_inv_norm for the cosine).
catalogue=ops.CompactCatalogue(...) serves both from the bf16 copy alone -- lists of up to 256 (pc_retrieve_list_grouped_bf16)
and diversified lists (pc_diversify_lists_bf16, pc_inv_norm_bf16); on this class ranks still need the fp32 catalogue.
CompactInference is the same object with rank_targets / evaluate_catalogue over the bf16 copy (pc_rank_grouped_bf16): it measures
what it serves, over the rounded table; rank_targets reads no fp32 features (evaluate_catalogue's dataset still wants a graph
that holds them: see the class).
recommend_capped_batch keeps at most `cap` products of one product group (a parent item, a brand, a seller) in a list, and
recommend_page_batch merges a query's K lists into one row under a per-type quota and that cap: one pc_cap_lists pass over
recommend_batch's own pool.  SimilarProducts.similar_capped_batch does the same for substitutes, without the query's variants.
recommend_basket_batch answers for a whole basket: the items' lists fused into one on the device (pc_fuse_lists), without the
basket's own products and the substitutes of any of them.  recommend_session_batch is the same for ragged sessions (a CSR of
items, no padding rows) with a weight per item -- recency, quantity, "purchased, so only ban it" -- (pc_fuse_sessions).
set_attributes / recommend_where_batch / similar_where_batch narrow a list by a per-QUERY predicate on per-product attributes -- a
band on a value (price), masks on 32 flag bits (regions, seller tiers) -- tested inside the long-list kernel
(pc_retrieve_list_grouped_where and its bf16 / biased twins): what set_eligible would serve per predicate, in one call.
score_moments / normalise="zscore" make the scores of different types comparable before a page or a basket merges them: the
mean and spread of every (query, type) slot's score over its whole type (pc_score_moments_grouped and its bf16 twin: the rank's
pass with two sums in the count's place), and z = (s - mean) / std on what recommend_batch serves.

SimilarProducts is the substitute side: the nearest products of a query under Euclidean distance over any [P, D] fp32 table
(Product2Vec's export), the grouped retrieval and rank with the per-product term -|e_p|^2 / 2 on the score
(pc_retrieve_topk_grouped_biased / pc_rank_grouped_biased), and hit@k / MRR over held-out similar pairs.  similar_list_batch
serves up to 256 neighbours (pc_retrieve_list_grouped_biased) and similar_capped_list_batch caps groups over such a pool.
CompactSimilarProducts is SimilarProducts over the bf16 copy of the table alone (pc_retrieve_list_grouped_bf16_biased,
pc_rank_grouped_bf16, pc_half_sq_norm_bias_bf16): distances to the stored rows, no fp32 table.
IndexedSimilarProducts serves its whole-catalogue scope through a k-means cell index (ops.build_cell_index): the same retrieval
over the products of a query's nearest cells, the probe lists of a query merged by pc_merge_lists.
IndexedCompactSimilarProducts is that index over the bf16 copy alone (ops.build_cell_index_bf16, pc_cell_means_bf16): the scan is
CompactSimilarProducts' entry, the index is built without the fp32 table, and a query probes up to 64 cells."""
import functools
import os
from typing import Any, Dict, List

import numpy as np
import torch

from . import ops
from .data import ComplementaryIndexDataset, DeviceBPG, IntBPG
from .metrics import Metrics
from .p_companion import PCompanion


def _refuse_tensor(what, name, wanted, t):
    """The refusal of an argument that is not the tensor asked for: '<what>: <name> must be <wanted>, got <shape> <dtype>' (the
    type's name for anything but a tensor)."""
    got = f"{tuple(t.shape)} {t.dtype}" if torch.is_tensor(t) else type(t).__name__
    raise ValueError(f"{what}: {name} must be {wanted}, got {got}")


def _check_group(what, group, cap):
    """cap as an int, and the shape of a product-group array (ops.cap_lists): cap >= 1, group None or a 1-D int32 tensor --
    ValueError before anything of the serving object is read."""
    cap = int(cap)
    if cap < 1:
        raise ValueError(f"{what}: cap must be at least 1, got {cap}")
    if group is not None and (not torch.is_tensor(group) or group.dtype != torch.int32 or group.dim() != 1):
        _refuse_tensor(what, "group", "None or a [P] int32 device tensor (the product's group, negative = ungrouped)", group)
    return cap


def _check_normalise(what, normalise):
    """normalise=None (the raw dot products) or "zscore"; anything else: ValueError, before the model runs."""
    if normalise is not None and normalise != "zscore":
        raise ValueError(f"{what}: normalise must be None or 'zscore', got {normalise!r}")


def _takes_normalise(method):
    """The keyword normalise=None | "zscore" of the five serving methods that end in recommend_batch's pool, in one place: the
    value is checked before anything of the method runs, None calls the method as it is (today's path, nothing set, nothing
    read), and "zscore" holds self._normalise for the length of the call, which recommend_batch -- the one place where served
    scores are made -- reads.  The keyword belongs to this wrapper, not to the method: inspect.signature follows
    functools.wraps to the method's own parameters, which the host tests of those methods pin; help() shows it in the
    docstrings.  The mode lives on the object: two threads that share one serving object must not mix normalised and raw
    calls."""
    @functools.wraps(method)
    def call(self, *args, normalise=None, **kwargs):
        _check_normalise(method.__name__, normalise)
        if normalise is None:
            return method(self, *args, **kwargs)
        before, self._normalise = self._normalise, normalise
        try:
            return method(self, *args, **kwargs)
        finally:
            self._normalise = before
    return call


class _CandidateFilters:
    """set_exclusions / set_eligible for a class that serves type-grouped candidates (PCompanionInference, SimilarProducts).
    The class provides device, type_idx [P] int32, _all_products = the unfiltered (type_rowptr, type_col), and the two hooks."""

    def _candidate_types(self):
        """(cand [P] int32: the type under which each product is a candidate, the number of types)"""
        return self.type_idx, self.bpg.n_types

    def _default_exclusions(self):
        """the device CSR set_exclusions() takes when none is given"""
        return self._graph["cv_rowptr"], self._graph["cv_col"]

    def set_exclusions(self, rowptr=None, col=None, include_self=True):
        """Keep named products out of what is served and ranked for a query: an exclusion set keyed by the QUERY product id.
        Default: the graph's own co-view CSR (co-viewed products are substitutes) and, with include_self, the query itself,
        through ops.exclusion_csr; rowptr / col: any device CSR over the products instead (a basket, say).  With a set installed
        recommend_batch, rank_targets and evaluate_catalogue go through pc_retrieve_topk_grouped_excluding /
        pc_rank_grouped_excluding with the query id as the row key of its K slots -- an uploaded IntBPG too: its arrays are on
        the device, and the per-row kernel has no filter.  set_exclusions(False) removes the set.  Once per catalogue, off the
        serving path.  (SimilarProducts: the default is the EMPTY CSR -- with include_self the query alone.)"""
        if rowptr is False:
            self.exclusions = None
            return self
        if (rowptr is None) != (col is None):
            raise ValueError("set_exclusions: pass rowptr and col together, or neither for the co-view graph")
        if rowptr is None:
            rowptr, col = self._default_exclusions()
        p = int(self.type_idx.shape[0])
        if rowptr.numel() != p + 1:
            raise ValueError(f"set_exclusions: the set is keyed by query id: rowptr must hold {p + 1} entries, got {rowptr.numel()}")
        self.exclusions = ops.exclusion_csr(rowptr.to(self.device), col.to(self.device), include_self=include_self, num_products=p)
        return self

    def set_eligible(self, mask=None):
        """Serve and rank over the eligible products only (in stock, not withdrawn): mask [P] bool on the device, None = all.
        Rebuilds type_rowptr / type_col over the eligible products (ops.type_csr on the filtered ids) and forms
        cand_type = where(mask, type_idx, -1); a held-out target that is not eligible gets rank -1."""
        cand, n_types = self._candidate_types()
        if mask is None:
            self.eligible, self.cand_type = None, cand
            self.type_rowptr, self.type_col = self._all_products
            return self
        p = int(self.type_idx.shape[0])
        if not torch.is_tensor(mask) or mask.dtype != torch.bool or tuple(mask.shape) != (p,):
            raise ValueError(f"set_eligible: expected a bool tensor of shape ({p},)")
        mask = mask.to(self.device)
        ids = torch.nonzero(mask).reshape(-1).to(torch.int32)
        rowptr, local = ops.type_csr(cand[ids.long()].contiguous(), n_types)
        self.type_rowptr, self.type_col = rowptr, ids[local.long()].contiguous()
        self.eligible = mask
        self.cand_type = torch.where(mask, cand, torch.full_like(cand, -1))
        return self

    attributes = None                          # (value [P] fp32 or None, flags [P] int32 or None): set_attributes

    def set_attributes(self, value=None, flags=None):
        """Install the per-product attributes that the *_where_batch methods filter on: value [P] float32 (a price, a rating, a
        delivery time) and / or flags [P] int32 read as 32 bits (ships-to-region bits, a seller tier), device tensors.  Once
        per catalogue, off the serving path; set_attributes() removes them.  Nothing is rebuilt: the predicate is per query
        (ops.RowWhere), the attributes are read by the list kernel as it scores."""
        p = int(self.type_idx.shape[0])
        for name, t, dtype in (("value", value, torch.float32), ("flags", flags, torch.int32)):
            if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != (p,)):
                raise ValueError(f"set_attributes: {name} must be a {dtype} tensor of shape ({p},), got "
                                 f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
        if value is None and flags is None:
            self.attributes = None
            return self
        self.attributes = tuple(None if t is None else t.to(self.device).contiguous() for t in (value, flags))
        return self

    def band_around(self, query_idx, below=0.5, above=2.0):
        """(lo, hi) = (value[q] * below, value[q] * above) as [B] fp32 device tensors: the band of the common case -- complements
        within 0.5x to 2x of the query's price.  Two multiplications."""
        if self.attributes is None or self.attributes[0] is None:
            raise ValueError("band_around: no per-product value is installed (set_attributes(value=...))")
        v = self.attributes[0][query_idx.to(self.device).long()]
        return v * below, v * above

    def _row_predicate(self, what, rows, lo, hi, need, deny):
        """The ops.RowWhere of `rows` queries from the installed attributes and the per-query arrays [rows] (a missing end of a
        band is infinite); ValueError where no attributes are installed, none of the four is given, or an array has no
        attribute to test -- before anything is computed."""
        if self.attributes is None:
            raise ValueError(f"{what}: no per-product attributes are installed (set_attributes)")
        if lo is None and hi is None and need is None and deny is None:
            raise ValueError(f"{what}: give at least one of lo, hi, need, deny (the unfiltered lists are the other methods')")
        value, flags = self.attributes
        band, masks = lo is not None or hi is not None, need is not None or deny is not None
        if band and value is None:
            raise ValueError(f"{what}: lo / hi bound the per-product value, and none is installed (set_attributes(value=...))")
        if masks and flags is None:
            raise ValueError(f"{what}: need / deny test the per-product flags, and none are installed (set_attributes(flags=...))")
        parts = {}
        for name, t, dtype in (("lo", lo, torch.float32), ("hi", hi, torch.float32), ("need", need, torch.int32),
                               ("deny", deny, torch.int32)):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != (rows,):
                raise ValueError(f"{what}: {name} must be a {dtype} tensor of one entry per query ({rows},), got "
                                 f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
            parts[name] = t.to(self.device).contiguous()
        if band:
            parts.setdefault("lo", torch.full((rows,), float("-inf"), device=self.device))
            parts.setdefault("hi", torch.full((rows,), float("inf"), device=self.device))
        return ops.RowWhere(value=value if band else None, flags=flags if masks else None, **parts)

    @staticmethod
    def _repeat_predicate(where, repeat):
        """`where` with every per-query entry repeated over `repeat` consecutive rows (a query's K slots), as _exclude_rows
        repeats the keys."""
        rep = lambda t: None if t is None else t.repeat_interleave(repeat).contiguous()
        return ops.RowWhere(where.value, where.flags, rep(where.lo), rep(where.hi), rep(where.need), rep(where.deny))

    def _group_covers(self, what, group):
        """a product-group array names every product of the catalogue (a shorter one would turn served ids into bad ids)"""
        if group is None:
            return
        p = int(self.type_idx.shape[0])
        if group.shape[0] != p:
            raise ValueError(f"{what}: group must hold one entry per product ({p}), got {group.shape[0]}")

    def _served_types(self, idx):
        """the served products' types: int64, idx's shape, -1 where idx is -1"""
        return torch.where(idx >= 0, self.type_idx[idx.clamp(min=0).long()].long(), -1)

    def _exclude_rows(self, query_idx, repeat=None):
        """The `exclude` triple of the grouped entries for rows keyed by their query's id -- `repeat` consecutive rows per query
        (its K slots, its probed cells), one if None; None when no set is installed."""
        if self.exclusions is None:
            return None
        if repeat is not None:
            query_idx = query_idx.repeat_interleave(repeat).contiguous()
        return (query_idx,) + self.exclusions

    def _excluded(self, query_idx, target_idx):
        """[B] bool: target_idx[b] is in query_idx[b]'s exclusion list (a bisection per pair, as vector operations; the lists
        are strictly ascending)."""
        ex_rowptr, ex_col = self.exclusions
        q = query_idx.long()
        lo, end = ex_rowptr[q].long(), ex_rowptr[q + 1].long()
        hi = end.clone()
        if ex_col.numel() == 0:
            return torch.zeros_like(q, dtype=torch.bool)
        y = target_idx.long()
        for _ in range(max(int(ex_col.numel()).bit_length(), 1)):
            mid = (lo + hi) >> 1
            below = (lo < hi) & (ex_col[mid.clamp(max=ex_col.numel() - 1)].long() < y)
            lo, hi = torch.where(below, mid + 1, lo), torch.where(below | (lo >= hi), hi, mid)
        return (lo < end) & (ex_col[lo.clamp(max=ex_col.numel() - 1)].long() == y)


class PCompanionInference(_CandidateFilters):
    catalogue = None                           # the bf16 copy that is served from (__init__: catalogue=); None: the fp32 features
    compact = None                             # the ops.CompactCatalogue behind `catalogue`, where one was given: long and
    #                                            diversified lists from the bf16 copy (None: today's bf16 / fp32 branches)

    def __init__(self, model, config, bpg: IntBPG, product_ids: List[str] = None, catalogue=None):
        """model: a trained PCompanion, or the path of a best_model.pth written by train.train
        (train.py:63-70 layout: 'model_state_dict' holds every tensor, including the frozen table).
        bpg: an IntBPG, or a DeviceBPG generated with world = 1 and with features (a sharded one holds a 1/world cyclic
        shard of the features and is refused, as in Product2Vec.generate_all_embeddings).
        catalogue: what the candidates are scored against.
          None            the graph's fp32 features (the parity setting).
          torch.bfloat16  ops.catalogue_bf16 of the graph's features, made here once.
          a [P, D] torch.bfloat16 device tensor: that copy, as it is; a DeviceBPG without features is then accepted.  This is
                          how a caller gets the memory back: the fp32 features belong to the graph object (and to whoever else
                          holds them -- the model's frozen table, say), and freeing them is the caller's business; this object
                          keeps no reference to them.
        With a bf16 catalogue recommend_batch (up to 16 per type) and recommend go through pc_retrieve_topk_grouped_bf16 for
        every kind of graph: the unrounded projected query against the ROUNDED table, so a list can differ from the fp32
        catalogue's where two products lie within bf16 rounding of each other.  set_exclusions / set_eligible work unchanged;
        lists above 16, rank_targets and evaluate_catalogue need the fp32 catalogue and raise ValueError.
          an ops.CompactCatalogue: its .table is the catalogue, checked and accepted as a given tensor is (a DeviceBPG
                          without features too), and the bf16 copy is then all this object needs for what it SERVES:
                          recommend_batch up to 16 as above (the same bits), from 17 to 256 through
                          pc_retrieve_list_grouped_bf16, and recommend_diverse_batch with its similarity over the bf16 rows
                          (pc_diversify_lists_bf16; the cosine from the object's .inv_norm) -- no fp32 features are read.
                          rank_targets and evaluate_catalogue still need the fp32 catalogue and raise ValueError."""
        self.config = config
        self.device = config.DEVICE
        self.bpg = bpg
        self.grouped = isinstance(bpg, DeviceBPG)
        if isinstance(catalogue, ops.CompactCatalogue):
            self.compact, catalogue = catalogue, catalogue.table
        given = torch.is_tensor(catalogue)
        if catalogue is not None and catalogue is not torch.bfloat16 and not given:
            raise ValueError(f"PCompanionInference: catalogue must be None (the fp32 features), torch.bfloat16 or a [P, D] "
                             f"torch.bfloat16 device tensor, got {catalogue!r}")
        if given:
            if catalogue.dtype != torch.bfloat16:
                raise ValueError(f"PCompanionInference: a catalogue tensor must be torch.bfloat16 (ops.catalogue_bf16), got "
                                 f"{catalogue.dtype}; the fp32 catalogue is catalogue=None")
            if catalogue.dim() != 2 or catalogue.shape[0] != bpg.num_products or catalogue.shape[1] not in (128, 256):
                raise ValueError(f"PCompanionInference: the catalogue must be [{bpg.num_products}, 128 or 256], got "
                                 f"{tuple(catalogue.shape)}")
            if not catalogue.is_cuda or not catalogue.is_contiguous():
                raise ValueError("PCompanionInference: the catalogue must be a contiguous device tensor")
        if self.grouped:
            if bpg.world != 1:
                raise ValueError(f"PCompanionInference: this DeviceBPG holds a cyclic 1/{bpg.world} shard of the features "
                                 f"(rank {bpg.rank}); serving needs the whole table on one device -- generate it with "
                                 "world = 1")
            if "features" not in bpg.arrays and not given:
                raise ValueError("PCompanionInference: the DeviceBPG was generated without features")
        if isinstance(model, (str, os.PathLike)):
            model = self._load_model(model)
        self.model = model.to(self.device)
        self.model.eval()
        self.product_ids = product_ids
        self._index = {pid: i for i, pid in enumerate(product_ids)} if product_ids is not None else None
        g = bpg.cuda(self.device)
        # the table the candidates are scored against: the fp32 features, or the bf16 copy (self.features is then None)
        if catalogue is None:
            self.features, self.catalogue = g["features"], None
        else:
            self.features, self.catalogue = None, (catalogue if given else ops.catalogue_bf16(g["features"]))
        self.type_idx = g["type_idx"]
        self._graph = g
        self.exclusions = None                 # (ex_rowptr, ex_col) keyed by query id: set_exclusions
        self.eligible = None                   # [P] bool: set_eligible
        self.cand_type = self.type_idx         # the type under which a product is a candidate (-1: none)
        if self.grouped:
            # the same CSR, built on the device: no host copy of type_idx, no host sort
            self.type_rowptr, self.type_col = ops.type_csr(self.type_idx, bpg.n_types)
            self._all_products = (self.type_rowptr, self.type_col)
            return
        # bpg.get_products_by_type(t) (bpg.py:40-43): products of type t in node order
        order = np.argsort(bpg.type_idx, kind="stable").astype(np.int32)
        counts = np.bincount(bpg.type_idx, minlength=bpg.n_types)
        rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.type_rowptr = torch.from_numpy(rowptr).to(self.device)
        self.type_col = torch.from_numpy(order).to(self.device)
        self._all_products = (self.type_rowptr, self.type_col)

    def _load_model(self, model_path):
        """Load trained model weights (inference.py:28-36)"""
        if not os.path.exists(model_path):
            raise FileNotFoundError(f"Model file not found: {model_path}")
        checkpoint = torch.load(model_path, map_location="cpu", weights_only=True)
        sd = checkpoint["model_state_dict"]
        model = PCompanion(self.config, sd["product_embeddings.weight"])
        model.load_state_dict(sd)
        return model

    def _to_index(self, query_id):
        if isinstance(query_id, (int, np.integer)):
            idx = int(query_id)
        elif self._index is not None:
            if query_id not in self._index:
                raise ValueError(f"Product ID {query_id} not found in BPG")      # inference.py:40-41
            idx = self._index[query_id]
        else:
            idx = int(str(query_id).lstrip("P"))
        if not 0 <= idx < self.bpg.num_products:
            raise ValueError(f"Product ID {query_id} not found in BPG")
        return idx

    @staticmethod
    def _list_length(num_recommendations):
        """num_recommendations as an int; above what pc_retrieve_list_grouped serves: ValueError, before the model runs."""
        n = int(num_recommendations)
        if n > ops.RETRIEVE_LIST_MAX_N:
            raise ValueError(f"recommend_batch: at most {ops.RETRIEVE_LIST_MAX_N} recommendations per (query, type), got {n}")
        return n

    _normalise = None                          # "zscore" while a call with normalise="zscore" runs (_takes_normalise)

    def _slot_rows(self, query_idx):
        """The model in eval mode on the queries -> (query_idx int32 on the device, complementary types [B, K] int64, the B K
        slots' projected embeddings [B K, D] and their types [B K] int32)."""
        query_idx = query_idx.to(self.device).to(torch.int32).contiguous()
        batch = {"query_idx": query_idx, "query_types": self.type_idx[query_idx.long()]}
        out = self.model(batch)
        types = out["complementary_types"]
        b, k = types.shape
        proj = out["projected_embeddings"].contiguous().reshape(b * k, -1)
        return query_idx, types, proj, types.to(torch.int32).reshape(-1).contiguous()

    def _moments(self, proj, row_types):
        """ops.score_moments_grouped of the slots over the installed type CSR and the table this object serves from"""
        table = self.catalogue if self.catalogue is not None else self.features
        return ops.score_moments_grouped(proj, row_types, self.type_rowptr, self.type_col, table)

    @torch.no_grad()
    def score_moments(self, query_idx: torch.Tensor):
        """The distribution behind recommend_batch's lists: (types [B, K] int64, count [B, K] int32, mean [B, K], std [B, K]
        fp32) -- for every slot the number of candidates of its predicted type and the mean and (population) standard deviation
        of the slot's score over ALL of them, one call of ops.score_moments_grouped over whatever table this object serves from:
        the fp32 features, a bare bf16 catalogue or an ops.CompactCatalogue's rows (CompactInference too).  The candidates are
        those of the installed type CSR, so set_eligible is honoured as it is for the lists.  The per-query exclusion lists
        (set_exclusions) are NOT subtracted: a handful of products among a whole type do not move its mean or spread.  Nothing is
        read back."""
        _, types, proj, row_types = self._slot_rows(query_idx)
        m = self._moments(proj, row_types)
        return types, m.count.reshape(types.shape), m.mean.reshape(types.shape), m.std.reshape(types.shape)

    @_takes_normalise
    @torch.no_grad()
    def recommend_batch(self, query_idx: torch.Tensor, num_recommendations: int = 10):
        """All queries at once.  Returns complementary_types [B,K] int64, product indices [B,K,n] int32
        (-1 past the end of a short type) and scores [B,K,n].  Up to 16 recommendations: the entries with a sorted list per
        thread; from 17 to ops.RETRIEVE_LIST_MAX_N (256): pc_retrieve_list_grouped, whatever the graph's kind -- an uploaded
        IntBPG's arrays are on the device, and the per-row kernel stops at 16.  A bf16 catalogue serves up to 16
        (pc_retrieve_topk_grouped_bf16); given as an ops.CompactCatalogue also 17 to 256 (pc_retrieve_list_grouped_bf16).
        normalise="zscore": the same model run and lists, the scores standardised per (query, type) --
        ops.standardise_scores against the moments of the slot's score over its whole type (score_moments, taken for all B K
        slots in one call) -- so that the lists of different types can be compared; a list keeps its order.  None: the raw dot
        products, today's path and bits."""
        n = self._list_length(num_recommendations)
        if self.catalogue is not None and n > 16 and self.compact is None:
            raise ValueError(f"recommend_batch: a bf16 catalogue serves at most 16 recommendations per (query, type), got {n}; "
                             "longer lists need the fp32 catalogue (catalogue=None)")
        query_idx, types, proj, row_types = self._slot_rows(query_idx)
        b, k = types.shape
        exclude = self._exclude_rows(query_idx, k)
        rows = (proj, row_types, self.type_rowptr, self.type_col)
        if self.catalogue is not None and n > 16:         # (a CompactCatalogue) the bf16 list entry
            idx, sc = ops.retrieve_list_grouped(*rows, self.catalogue, n, exclude=exclude)
        elif self.catalogue is not None:                  # (n <= 16) the bf16 entry, whatever the graph's kind
            idx, sc = ops.retrieve_topk_grouped(*rows, self.catalogue, n, exclude=exclude)
        elif n > 16:                                      # (RG_MAX_N / RMAX_N: the entries below refuse 17)
            idx, sc = ops.retrieve_list_grouped(*rows, self.features, n, exclude=exclude)
        elif exclude is not None or self.grouped:
            # (the per-row kernel has no filter: with a set the grouped search, whatever the graph's kind)
            idx, sc = ops.retrieve_topk_grouped(*rows, self.features, n, exclude=exclude)
        else:
            idx, sc = ops.retrieve_topk(*rows, self.features, n)
        if self._normalise is not None:
            m = self._moments(proj, row_types)
            sc = ops.standardise_scores(sc, m.mean[:, None], m.std[:, None], m.count[:, None])
        return types, idx.reshape(b, k, -1), sc.reshape(b, k, -1)

    @torch.no_grad()
    def recommend_where_batch(self, query_idx: torch.Tensor, num_recommendations: int = 10, lo: torch.Tensor = None,
                              hi: torch.Tensor = None, need: torch.Tensor = None, deny: torch.Tensor = None):
        """recommend_batch's lists over the products that pass a per-QUERY predicate on the installed attributes
        (set_attributes): lo / hi [B] float32 pass product p iff lo[b] <= value[p] <= hi[b] (band_around gives the band around
        the query's own value; a missing end is infinite), need / deny [B] int32 pass it iff (flags[p] & need[b]) == need[b] and
        (flags[p] & deny[b]) == 0.  The per-query arrays are repeated over the query's K slots as the exclusion keys are; the
        exclusions and the eligibility installed on this object apply as in recommend_batch.  One call of
        ops.retrieve_list_grouped_where for any 1 <= num_recommendations <= 256: what recommend_batch would serve under
        set_eligible(mask of the predicate), bit for bit, for predicates that differ per query.  Returns recommend_batch's
        triple.  Served from the fp32 features or an ops.CompactCatalogue; a bare bf16 catalogue stops at 16, as it does for
        recommend_batch.  ValueError before the model runs where no attributes are installed or none of the four is given."""
        n = self._list_length(num_recommendations)
        if n < 1:
            raise ValueError(f"recommend_where_batch: at least 1 recommendation per (query, type), got {n}")
        if self.catalogue is not None and n > 16 and self.compact is None:
            raise ValueError(f"recommend_where_batch: a bf16 catalogue serves at most 16 recommendations per (query, type), got "
                             f"{n}; longer lists need the fp32 catalogue (catalogue=None) or an ops.CompactCatalogue")
        where = self._row_predicate("recommend_where_batch", int(query_idx.shape[0]), lo, hi, need, deny)
        query_idx = query_idx.to(self.device).to(torch.int32).contiguous()
        batch = {"query_idx": query_idx, "query_types": self.type_idx[query_idx.long()]}
        out = self.model(batch)
        types = out["complementary_types"]
        b, k = types.shape
        proj = out["projected_embeddings"].contiguous().reshape(b * k, -1)
        row_types = types.to(torch.int32).reshape(-1).contiguous()
        table = self.catalogue if self.catalogue is not None else self.features
        idx, sc = ops.retrieve_list_grouped_where(proj, row_types, self.type_rowptr, self.type_col, table, n,
                                                  self._repeat_predicate(where, k), exclude=self._exclude_rows(query_idx, k))
        return types, idx.reshape(b, k, -1), sc.reshape(b, k, -1)

    _inv_norm = None                           # ops.inv_norm of the fp32 features: recommend_diverse_batch, formed on first use

    @torch.no_grad()
    def recommend_diverse_batch(self, query_idx: torch.Tensor, num_recommendations: int = 10, pool: int = 64,
                                diversity: float = 0.3, similarity: str = "cosine"):
        """recommend_batch's lists re-ranked for diversity inside a type: the pool is recommend_batch(query_idx, pool) itself --
        its exclusions, eligibility, catalogue and choice of retrieval entry --, and ops.diversify_lists picks the
        num_recommendations products to show from it by greedy maximal marginal relevance with lam = 1 - diversity: every pick
        is the best of relevance weighed against its largest similarity to the products already picked.  similarity: "cosine"
        (the dot product of the fp32 features' rows times ops.inv_norm of both, formed once on first use) or "dot" (no scale).
        diversity = 0 is recommend_batch(query_idx, num_recommendations), bit for bit, wherever both go through the grouped
        entries (an uploaded IntBPG without exclusions serves up to 16 through the per-row kernel, whose sums run in another
        order: there it is the same list up to that kernel's last bits).  Returns recommend_batch's triple
        (types [B, K], idx [B, K, n], score [B, K, n]): the scores are the pool's relevance scores, in pick order.
        1 <= num_recommendations <= pool <= ops.DIVERSIFY_MAX_POOL and 0 <= diversity <= 1, checked before the model runs; the
        similarity reads the fp32 features, so a bf16 catalogue needs a graph that still holds them and bounds the pool at
        what it serves (16).  With an ops.CompactCatalogue neither holds: the pool (up to 256) and the similarity both come from
        the bf16 rows (ops.diversify_lists_bf16; "cosine": the catalogue's .inv_norm, the factors of the rounded rows), and the
        result is bit for bit ops.diversify_lists over the widened table."""
        n, pool = int(num_recommendations), int(pool)
        if not 1 <= n <= pool <= ops.DIVERSIFY_MAX_POOL:
            raise ValueError(f"recommend_diverse_batch: need 1 <= num_recommendations <= pool <= {ops.DIVERSIFY_MAX_POOL}, got "
                             f"num_recommendations {n} and pool {pool}")
        diversity = float(diversity)
        if not 0.0 <= diversity <= 1.0:
            raise ValueError(f"recommend_diverse_batch: diversity must be in [0, 1], got {diversity}")
        if similarity not in ("cosine", "dot"):
            raise ValueError(f"recommend_diverse_batch: similarity must be 'cosine' or 'dot', got {similarity!r}")
        table = self._similarity_table("recommend_diverse_batch")
        types, idx, sc = self.recommend_batch(query_idx, pool)
        b, k, m = idx.shape
        idx, sc = self._rerank(idx.reshape(b * k, m), sc.reshape(b * k, m), table, n, diversity, similarity)
        return types, idx.reshape(b, k, n), sc.reshape(b, k, n)

    def _similarity_table(self, what):
        """The fp32 table the re-rank's similarity reads -- None with an ops.CompactCatalogue, whose bf16 rows serve it; a
        graph without fp32 features and without one: ValueError, before the model runs."""
        if self.compact is not None:
            return None
        table = self.features if self.features is not None else self._graph.get("features")
        if table is None:
            raise ValueError(f"{what}: the similarity is taken over the fp32 features, and this graph was "
                             "generated without them (the bf16 catalogue alone cannot serve diversified lists)")
        return table

    def _rerank(self, idx, sc, table, n, diversity, similarity):
        """The greedy MMR pick of n from the pools idx / sc [R, m] (recommend_diverse_batch, recommend_capped_batch): the choice
        between ops.diversify_lists_bf16 over a CompactCatalogue's rows and ops.diversify_lists over `table`
        (_similarity_table), and the cosine's scale."""
        if self.compact is not None:                      # the similarity from the bf16 copy alone
            return ops.diversify_lists_bf16(idx, sc, self.catalogue, n, 1.0 - diversity,
                                            scale=self.compact.inv_norm if similarity == "cosine" else None)
        scale = None
        if similarity == "cosine":
            if self._inv_norm is None:
                self._inv_norm = ops.inv_norm(table)          # once per catalogue
            scale = self._inv_norm
        return ops.diversify_lists(idx, sc, table, n, 1.0 - diversity, scale=scale)

    @_takes_normalise
    @torch.no_grad()
    def recommend_capped_batch(self, query_idx: torch.Tensor, num_recommendations: int = 10, group: torch.Tensor = None,
                               cap: int = 1, pool: int = 64, diversity: float = None, similarity: str = "cosine"):
        """recommend_batch's lists with at most `cap` products of one product group (a parent item, a brand, a seller) per
        list.  group [P] int32 on the device: the product's group, negative = ungrouped and never capped.  The pool is
        recommend_batch(query_idx, pool) itself -- its exclusions, eligibility, catalogue and choice of retrieval entry --, and
        ops.cap_lists walks it in serving order and keeps a product while its group has room.  diversity=None: the first
        num_recommendations kept products.  A diversity in [0, 1]: every kept product of the pool (ops.cap_lists with n = pool),
        then exactly recommend_diverse_batch's re-rank of that pool -- the same entry, similarity and scale; the cap is
        enforced on the pool, the re-rank then orders what is left.  Returns recommend_batch's triple (types [B, K], idx
        [B, K, n], score [B, K, n]), the scores the pool's own bits, -1 / -inf where the capped pool holds fewer than
        num_recommendations products: the cap is on a POOL, and a pool that is mostly one group gives a short list -- take a
        longer pool.  1 <= num_recommendations <= pool <= ops.CAP_LISTS_MAX_POOL and cap >= 1, checked before the model runs.
        group=None and diversity=None is recommend_batch(query_idx, num_recommendations), bit for bit, wherever the pool comes
        through a grouped entry.  normalise="zscore": the pool is recommend_batch(query_idx, pool, normalise="zscore") -- the
        cap and the re-rank see the standardised scores and return them; None: today's path and bits."""
        n, pool = int(num_recommendations), int(pool)
        if not 1 <= n <= pool <= ops.CAP_LISTS_MAX_POOL:
            raise ValueError(f"recommend_capped_batch: need 1 <= num_recommendations <= pool <= {ops.CAP_LISTS_MAX_POOL}, got "
                             f"num_recommendations {n} and pool {pool}")
        cap = _check_group("recommend_capped_batch", group, cap)
        table = None
        if diversity is not None:
            diversity = float(diversity)
            if not 0.0 <= diversity <= 1.0:
                raise ValueError(f"recommend_capped_batch: diversity must be None or in [0, 1], got {diversity}")
            if similarity not in ("cosine", "dot"):
                raise ValueError(f"recommend_capped_batch: similarity must be 'cosine' or 'dot', got {similarity!r}")
            table = self._similarity_table("recommend_capped_batch")
        self._group_covers("recommend_capped_batch", group)
        types, idx, sc = self.recommend_batch(query_idx, pool)
        b, k, m = idx.shape
        idx, sc = idx.reshape(b * k, m), sc.reshape(b * k, m)
        if diversity is None:
            idx, sc = ops.cap_lists(idx, sc, n, group, cap)
        else:
            idx, sc = ops.cap_lists(idx, sc, m, group, cap)                       # every kept product; -1 slots are no candidates
            idx, sc = self._rerank(idx, sc, table, n, diversity, similarity)
        return types, idx.reshape(b, k, n), sc.reshape(b, k, n)

    @_takes_normalise
    @torch.no_grad()
    def recommend_page_batch(self, query_idx: torch.Tensor, num_recommendations: int = 10, per_type: int = 4,
                             group: torch.Tensor = None, cap: int = 1):
        """One row per query across its K predicted complementary types -- what a widget shows: (idx [B, n] int32, score
        [B, n] fp32, types [B, n] int64 = the product's type, -1 where idx is -1).  The K lists of
        recommend_batch(query_idx, per_type) side by side are one pool of K per_type products, and ONE ops.cap_lists call
        merges it under the serving order (score descending, product index ascending): the per-type quota is the pool's own
        length -- no type can place more than per_type products --, and the group cap (group [P] int32, negative = ungrouped;
        None: no cap) holds across the whole page.  The scores of different types are compared AS THEY ARE: each is the dot
        product of that type's projected query with the product's features, and nothing normalises one type against another --
        a type whose projections score higher takes the head of the page.  Needs K per_type <= ops.CAP_LISTS_MAX_POOL and
        1 <= num_recommendations <= K per_type (and cap >= 1), checked before the model runs; -1 / -inf where fewer products
        are kept.  normalise="zscore" is the remedy: the pool is recommend_batch(query_idx, per_type, normalise="zscore"), every
        score standardised against the mean and spread of its own (query, type) slot over the whole type, so the page is
        ordered by how exceptional a product is for its slot and no longer by which type projects loudest; the returned scores
        are the standardised ones.  None: today's path and bits."""
        n, per_type, k = int(num_recommendations), int(per_type), int(self.config.NUM_COMP_TYPES)
        if per_type < 1 or k * per_type > ops.CAP_LISTS_MAX_POOL:
            raise ValueError(f"recommend_page_batch: need 1 <= per_type and K * per_type <= {ops.CAP_LISTS_MAX_POOL}, got K = {k} "
                             f"and per_type {per_type}")
        if not 1 <= n <= k * per_type:
            raise ValueError(f"recommend_page_batch: need 1 <= num_recommendations <= K * per_type = {k * per_type}, got {n}")
        cap = _check_group("recommend_page_batch", group, cap)
        self._group_covers("recommend_page_batch", group)
        _, idx, sc = self.recommend_batch(query_idx, per_type)
        b = idx.shape[0]
        idx, sc = ops.cap_lists(idx.reshape(b, -1), sc.reshape(b, -1), n, group, cap)
        return idx, sc, self._served_types(idx)

    @_takes_normalise
    @torch.no_grad()
    def recommend_basket_batch(self, basket: torch.Tensor, num_recommendations: int = 10, per_item: int = 8,
                               combine: str = "sum"):
        """What goes with ALL the products of a basket: (idx [B, n] int32, score [B, n] fp32, types [B, n] int64 = the
        product's type, -1 where idx is -1, support [B, n] int32).  basket [B, I] int32: the product ids of each basket's items,
        -1 = no item (padding).  Every item is served as a query of its own -- recommend_batch(items, per_item): its catalogue,
        its per-item exclusions and eligibility, its choice of retrieval entry and its refusals (a bare bf16 catalogue stops at
        per_item 16) --, the I rows of K per_item slots are one pool, and ONE ops.fuse_lists call fuses it: a product that
        several items (or several types of one item) suggested is one product, its scores met under `combine` ("sum": added,
        the largest first, sequential fp32 -- a product many items agree on rises; "max": its best score, a dedupe), support =
        the number of lists that offered it; the basket's own items are never served, and with an exclusion set installed
        (set_exclusions) neither is a product in the set of ANY item, whichever item's list offered it.  Served under
        (fused score descending, product index ascending), -1 / -inf / -1 / 0 where fewer products are left.  Needs
        I K per_item <= ops.FUSE_LISTS_MAX_POOL and 1 <= num_recommendations <= min(I K per_item, ops.FUSE_LISTS_MAX_N), checked
        before the model runs.  A padding slot still costs a retrieval row (it is served for product 0 and dropped by the
        fusion), so bucket baskets by length.  Nothing is read back.  normalise="zscore": the items are served by
        recommend_batch(items, per_item, normalise="zscore"), so the fusion adds (or takes the largest of) standardised scores
        and no type's scale outweighs the agreement of several items; None: today's path and bits."""
        n, per_item, k = int(num_recommendations), int(per_item), int(self.config.NUM_COMP_TYPES)
        if not torch.is_tensor(basket) or basket.dim() != 2 or basket.dtype != torch.int32 or basket.shape[1] < 1:
            _refuse_tensor("recommend_basket_batch", "basket", "a [B, I] int32 tensor with I >= 1 (-1 = no item)", basket)
        b, items = basket.shape
        if per_item < 1 or items * k * per_item > ops.FUSE_LISTS_MAX_POOL:
            raise ValueError(f"recommend_basket_batch: need 1 <= per_item and I * K * per_item <= {ops.FUSE_LISTS_MAX_POOL}, got "
                             f"I = {items}, K = {k} and per_item {per_item}")
        most = min(items * k * per_item, ops.FUSE_LISTS_MAX_N)
        if not 1 <= n <= most:
            raise ValueError(f"recommend_basket_batch: need 1 <= num_recommendations <= min(I * K * per_item, "
                             f"{ops.FUSE_LISTS_MAX_N}) = {most}, got {n}")
        if combine not in ("sum", "max"):
            raise ValueError(f"recommend_basket_batch: combine must be 'sum' or 'max', got {combine!r}")
        basket = basket.to(self.device).contiguous()
        p = int(self.type_idx.shape[0])
        # (padding is served for product 0, an id outside the catalogue for the nearest one inside: the fusion drops both rows)
        _, idx, sc = self.recommend_batch(basket.reshape(-1).clamp(0, p - 1), per_item)
        idx, sc, support = ops.fuse_lists(idx.reshape(b, items, -1), sc.reshape(b, items, -1), n, combine, source=basket,
                                          exclude=self.exclusions, num_products=p)
        return idx, sc, self._served_types(idx), support

    @_takes_normalise
    @torch.no_grad()
    def recommend_session_batch(self, items: torch.Tensor, seg_rowptr: torch.Tensor, num_recommendations: int = 10,
                                per_item: int = 8, weight: torch.Tensor = None, combine: str = "sum", max_items: int = None):
        """recommend_basket_batch for RAGGED sessions with a weight per item: (idx [B, n] int32, score [B, n] fp32, types
        [B, n] int64 = the product's type, -1 where idx is -1, support [B, n] int32).  items [R] int32: the product ids of all
        sessions' items, one after the other, each session's oldest first; seg_rowptr [B + 1] int32: session b owns
        items[seg_rowptr[b]:seg_rowptr[b + 1]] (an empty session is served as all padding).  There are no padding rows: ONE
        recommend_batch(items.clamp(0, P - 1), per_item) serves the R real items -- its catalogue, its per-item exclusions and
        eligibility, its choice of retrieval entry and its refusals (a bare bf16 catalogue stops at per_item 16) --, and ONE
        ops.fuse_sessions call (source=items, exclude=the installed exclusion set) fuses each session's rows of K per_item
        slots as recommend_basket_batch fuses a basket's: the same ids, score bits and supports as that method serves for the
        sessions padded with -1.  weight [R] fp32 (None: every weight is 1): a slot's score is multiplied by its item's weight
        (one rounded fp32 product) before the fusion; an item whose weight is not finite and > 0 -- 0: "purchased, so only
        ban it" -- offers nothing, but it and its excluded products are still kept out of the list.  Recency decay is a torch
        one-liner that does not synchronise, e.g. for half a point per step back from the session's last item:
            length = (seg_rowptr[1:] - seg_rowptr[:-1]).long()
            age = seg_rowptr[1:].repeat_interleave(length, output_size=R) - 1 - torch.arange(R, device=length.device)
            weight = torch.pow(0.5, age.float())
        Only the last min(1024 // (K per_item), max_items) items of a session offer (max_items None: no cap); every item
        bans.  Needs K per_item <= ops.FUSE_SESSIONS_MAX_POOL and 1 <= num_recommendations <= ops.FUSE_SESSIONS_MAX_N, checked
        before the model runs.  Nothing is read back.  normalise="zscore": the items are served by recommend_batch(...,
        normalise="zscore") and the weights multiply standardised scores, as in recommend_basket_batch; None: today's path and
        bits."""
        n, per_item, k = int(num_recommendations), int(per_item), int(self.config.NUM_COMP_TYPES)
        if not torch.is_tensor(items) or items.dim() != 1 or items.dtype != torch.int32:
            _refuse_tensor("recommend_session_batch", "items", "a [R] int32 tensor", items)
        if (not torch.is_tensor(seg_rowptr) or seg_rowptr.dim() != 1 or seg_rowptr.dtype != torch.int32
                or seg_rowptr.numel() < 1):
            _refuse_tensor("recommend_session_batch", "seg_rowptr", "a [B + 1] int32 tensor", seg_rowptr)
        r = items.shape[0]
        if weight is not None and (not torch.is_tensor(weight) or weight.dtype != torch.float32
                                   or tuple(weight.shape) != (r,)):
            _refuse_tensor("recommend_session_batch", "weight", f"a [R = {r}] float32 tensor", weight)
        if per_item < 1 or k * per_item > ops.FUSE_SESSIONS_MAX_POOL:
            raise ValueError(f"recommend_session_batch: need 1 <= per_item and K * per_item <= {ops.FUSE_SESSIONS_MAX_POOL}, "
                             f"got K = {k} and per_item {per_item}")
        if not 1 <= n <= ops.FUSE_SESSIONS_MAX_N:
            raise ValueError(f"recommend_session_batch: need 1 <= num_recommendations <= {ops.FUSE_SESSIONS_MAX_N}, got {n}")
        if combine not in ("sum", "max"):
            raise ValueError(f"recommend_session_batch: combine must be 'sum' or 'max', got {combine!r}")
        if max_items is not None and int(max_items) < 0:
            raise ValueError(f"recommend_session_batch: max_items must be None or at least 0 (0: no cap), got {max_items}")
        items = items.to(self.device).contiguous()
        seg_rowptr = seg_rowptr.to(self.device).contiguous()
        if weight is not None:
            weight = weight.to(self.device).contiguous()
        p = int(self.type_idx.shape[0])
        # (an id outside the catalogue is served for the nearest one inside: the fusion lets its row offer nothing)
        _, idx, sc = self.recommend_batch(items.clamp(0, p - 1), per_item)
        idx, sc, support = ops.fuse_sessions(idx.reshape(r, k * per_item), sc.reshape(r, k * per_item), seg_rowptr, n, combine, source=items,
                                             weight=weight, exclude=self.exclusions, num_products=p, max_items=max_items)
        return idx, sc, self._served_types(idx), support

    def _rank_guard(self, what):
        """rank_targets and evaluate_catalogue ask here first: a bf16 catalogue is refused, before the model runs or the
        dataset is looked at (CompactInference, which ranks over the bf16 table, lets it pass)."""
        if self.catalogue is not None:
            raise ValueError(f"{what}: the rank kernels read the fp32 catalogue (catalogue=None); a bf16 catalogue serves "
                             "recommend_batch / recommend up to 16 per type")

    def _rank_entry(self):
        """(the ops function the ranks go through, the table it reads)"""
        return ops.rank_grouped, self.features

    @torch.no_grad()
    def rank_targets(self, query_idx: torch.Tensor, target_idx: torch.Tensor, take: torch.Tensor = None):
        """Where does target_idx[b] stand in what is served for query_idx[b]?  The model runs in eval mode on the queries;
        slot[b] = the k whose predicted complementary type is the target's type (the top-K types are distinct: at most
        one), -1 if none is; rank[b] = the number of products of that type that slot's projected embedding scores above
        the target (equal scores: the lower product index first) -- the target's position in recommend_batch's list of
        that slot, were the list the whole type -- or -1 when slot[b] is -1.  With set_exclusions / set_eligible the products
        they keep out are not counted, and a target they keep out has rank -1 (its slot stays).  A target outside the catalogue has no type:
        slot -1, rank -1.  `take` [B] bool (optional): rows that are False get slot -1 / rank -1 and cost no search.
        Returns (slot int32 [B], rank int32 [B]) on the device; nothing is read back."""
        self._rank_guard("rank_targets")
        rank_grouped, table = self._rank_entry()
        rows = self._target_rows("rank_targets", query_idx, target_idx, take, table)
        if rows is None:
            e = torch.empty(0, dtype=torch.int32, device=self.device)
            return e, e.clone()
        query_idx, target_idx, slot, proj, row_type = rows
        exclude = self._exclude_rows(query_idx)
        if exclude is not None:
            # a target in the query's list, or not eligible: -1 from the entry itself
            rank, _ = rank_grouped(proj, row_type, target_idx, self.type_rowptr, self.type_col, table, exclude=exclude,
                                   cand_type=self.cand_type)
            return slot, rank
        rank, _ = rank_grouped(proj, row_type, target_idx, self.type_rowptr, self.type_col, table)
        if self.eligible is not None:
            kept = self.eligible[target_idx.long().clamp(0, table.shape[0] - 1)]
            rank = torch.where(kept, rank, torch.full_like(rank, -1))
        return slot, rank

    def _target_rows(self, what, query_idx, target_idx, take, table):
        """rank_targets' rows: the model in eval mode on the queries and the slot whose predicted type is the target's ->
        (query_idx, target_idx -- int32 on the device --, slot [B] int32, proj [B, D] of that slot, row_type [B] int32, -1
        where no slot matches or `take` is False); None for no pair."""
        query_idx = query_idx.to(self.device).to(torch.int32).contiguous()
        target_idx = target_idx.to(self.device).to(torch.int32).contiguous()
        if query_idx.dim() != 1 or query_idx.shape != target_idx.shape:
            raise ValueError(f"{what}: query_idx and target_idx must be 1-D and of equal length")
        b = query_idx.shape[0]
        if b == 0:
            return None
        out = self.model({"query_idx": query_idx, "query_types": self.type_idx[query_idx.long()]})
        types = out["complementary_types"]                                        # [B, K], distinct in a row
        inside = (target_idx >= 0) & (target_idx < table.shape[0])
        target_type = self.type_idx[target_idx.long().clamp(0, table.shape[0] - 1)].long()
        match = (types == target_type[:, None]) & inside[:, None]
        if take is not None:
            match &= take.to(self.device).bool()[:, None]
        found = match.any(1)
        k = match.to(torch.int32).argmax(1)
        slot = torch.where(found, k, torch.full_like(k, -1)).to(torch.int32)
        proj = out["projected_embeddings"][torch.arange(b, device=self.device), k].contiguous()      # [B, D]
        row_type = torch.where(found, target_type, torch.full_like(target_type, -1)).to(torch.int32)
        return query_idx, target_idx, slot, proj, row_type

    @torch.no_grad()
    def rank_targets_where(self, query_idx: torch.Tensor, target_idx: torch.Tensor, lo: torch.Tensor = None,
                           hi: torch.Tensor = None, need: torch.Tensor = None, deny: torch.Tensor = None,
                           take: torch.Tensor = None):
        """rank_targets under a per-QUERY predicate on the installed attributes (set_attributes; lo / hi / need / deny [B] as
        in recommend_where_batch): rank[b] = the number of products of the matched slot's type that PASS query b's predicate
        and that the slot's projected embedding scores above the target -- the target's position in recommend_where_batch's
        list of that slot, were the list the whole type: rank < n exactly when recommend_where_batch(query, n, ...) holds the
        target at that position.  The installed exclusions and eligibility apply as in rank_targets; a target they keep out,
        or that fails its own query's predicate, keeps its slot and has rank -1.  One call of ops.rank_grouped_where, over the
        fp32 features (CompactInference: the bf16 copy).  Returns (slot int32 [B], rank int32 [B]) on the device.  ValueError
        before the model runs where no attributes are installed, none of the four is given, or an array has no attribute."""
        self._rank_guard("rank_targets_where")
        where = self._row_predicate("rank_targets_where", int(query_idx.shape[0]) if query_idx.dim() else -1, lo, hi, need, deny)
        table = self._rank_entry()[1]
        rows = self._target_rows("rank_targets_where", query_idx, target_idx, take, table)
        if rows is None:
            e = torch.empty(0, dtype=torch.int32, device=self.device)
            return e, e.clone()
        query_idx, target_idx, slot, proj, row_type = rows
        exclude = self._exclude_rows(query_idx)
        if exclude is not None:
            rank, _ = ops.rank_grouped_where(proj, row_type, target_idx, self.type_rowptr, self.type_col, table, where,
                                             exclude=exclude, cand_type=self.cand_type)
            return slot, rank
        rank, _ = ops.rank_grouped_where(proj, row_type, target_idx, self.type_rowptr, self.type_col, table, where)
        if self.eligible is not None:
            kept = self.eligible[target_idx.long().clamp(0, table.shape[0] - 1)]
            rank = torch.where(kept, rank, torch.full_like(rank, -1))
        return slot, rank

    def _fails_predicate(self, target_idx, parts):
        """[B] bool: target_idx[b] fails the predicate `parts` (lo / hi / need / deny [B], any of them) of its own pair --
        ops.RowWhere's test on value[y] / flags[y] as vector operations: two inclusive fp32 compares (a NaN passes nothing),
        two masks."""
        value, flags = self.attributes
        y = target_idx.long().clamp(0, int(self.type_idx.shape[0]) - 1)
        fails = torch.zeros_like(y, dtype=torch.bool)
        if parts.get("lo") is not None:
            fails |= ~(parts["lo"].to(self.device) <= value[y])
        if parts.get("hi") is not None:
            fails |= ~(value[y] <= parts["hi"].to(self.device))
        if parts.get("need") is not None:
            need = parts["need"].to(self.device)
            fails |= (flags[y] & need) != need
        if parts.get("deny") is not None:
            fails |= (flags[y] & parts["deny"].to(self.device)) != 0
        return fails

    def _predicate_parts(self, what, predicate, query_idx):
        """predicate(query_idx) as a dict with any of lo, hi, need, deny (ValueError for anything else)"""
        parts = predicate(query_idx)
        if not isinstance(parts, dict) or not set(parts) <= {"lo", "hi", "need", "deny"}:
            raise ValueError(f"{what}: predicate(query_idx) must return a dict with any of lo, hi, need, deny, got "
                             f"{sorted(parts) if isinstance(parts, dict) else type(parts).__name__}")
        return parts

    def evaluate_catalogue_where(self, dataset: ComplementaryIndexDataset, predicate, ks=(1, 3, 10, 100),
                                 chunk: int = 65536) -> Dict[str, Any]:
        """evaluate_catalogue of what recommend_where_batch serves: predicate(query_idx) -- query_idx an int32 device vector, a
        chunk's queries -- returns a dict with any of lo, hi, need, deny ([chunk] tensors), for instance
        lambda q: dict(zip(("lo", "hi"), inf.band_around(q))); the chunks go through rank_targets_where.  Returns
        evaluate_catalogue's dict: hit@k for k <= 256 is the share of the +1 pairs whose target is among
        recommend_where_batch(query, k, **predicate(query))'s lists.  "filtered_targets" is always there and also counts the
        pairs whose target fails its own query's predicate (value[y] / flags[y] tested in torch): such a pair is a miss."""
        what = "evaluate_catalogue_where"
        self._rank_guard(what)
        if self.attributes is None:
            raise ValueError(f"{what}: no per-product attributes are installed (set_attributes)")
        if not callable(predicate):
            raise ValueError(f"{what}: predicate must be a callable of the chunk's query ids, got {type(predicate).__name__}")
        return self._evaluate(what, dataset, ks, chunk, predicate)

    def evaluate_catalogue(self, dataset: ComplementaryIndexDataset, ks=(1, 3, 10, 100), chunk: int = 65536) -> Dict[str, Any]:
        """Are the held-out complements among what is served?  `dataset`: a ComplementaryIndexDataset over this object's
        graph, normally mode "test" (the 10 % of the labelled pairs no other phase reads); only its +1 pairs take part.
        Chunks of `chunk` pairs go through rank_targets into two device vectors; Metrics.catalogue_metrics folds them
        (integer counts, one float64 reciprocal-rank sum in a fixed order) and reads back once.  Over a DeviceBPG the -1
        pairs stay in the chunks as rows that cost no search, so nothing is compacted or counted on the host.
        Returns {"pairs", "type_hit", "hit@k" for k in ks, "mrr", "median_rank"}: hit@k is the share of all +1 pairs
        whose target is among the first k products of its type under the matched slot (k <= 256: among
        recommend_batch(query, k)'s lists), 0 for a pair whose type no slot predicted.  The candidates are every product
        of the type, the query included, as in serving.  With set_exclusions / set_eligible the candidates are what is then
        served; a pair whose target the filters keep out (it is in its query's list, or not eligible) is a miss -- it keeps its
        slot, its rank is -1 -- and the dict gains "filtered_targets", the number of such pairs."""
        return self._evaluate("evaluate_catalogue", dataset, ks, chunk)

    def _evaluate(self, what, dataset, ks, chunk, predicate=None):
        """evaluate_catalogue; with a predicate evaluate_catalogue_where (the chunks through rank_targets_where)"""
        self._rank_guard(what)
        bpg = self.bpg
        if isinstance(bpg, DeviceBPG) and bpg.world != 1:
            raise ValueError(f"{what}: this DeviceBPG holds a cyclic 1/{bpg.world} shard of the features")
        if not isinstance(dataset, ComplementaryIndexDataset) or dataset.bpg is not bpg:
            raise ValueError(f"{what}: the dataset was built over another graph than this object serves")
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"{what}: chunk must be positive")
        pairs = dataset.pairs
        if not torch.is_tensor(pairs):
            pairs = np.asarray(pairs)
            pairs = torch.from_numpy(np.ascontiguousarray(pairs[pairs[:, 2] == 1], dtype=np.int32))
        if pairs.shape[0] == 0:
            raise ValueError(f"{what}: the dataset holds no +1 pair")
        pairs = pairs.to(self.device)
        n = pairs.shape[0]
        take = pairs[:, 2] == 1
        slot = torch.empty(n, dtype=torch.int32, device=self.device)
        rank = torch.empty(n, dtype=torch.int32, device=self.device)
        filtering = self.exclusions is not None or self.eligible is not None or predicate is not None
        filtered = torch.zeros((), dtype=torch.int64, device=self.device)
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            if predicate is None:
                slot[lo:hi], rank[lo:hi] = self.rank_targets(pairs[lo:hi, 0], pairs[lo:hi, 1], take[lo:hi])
            else:
                parts = self._predicate_parts(what, predicate, pairs[lo:hi, 0].contiguous())
                slot[lo:hi], rank[lo:hi] = self.rank_targets_where(pairs[lo:hi, 0], pairs[lo:hi, 1], take=take[lo:hi], **parts)
            if filtering:
                q, y = pairs[lo:hi, 0], pairs[lo:hi, 1]
                out = torch.zeros_like(take[lo:hi])
                if self.exclusions is not None:
                    out |= self._excluded(q, y)
                if self.eligible is not None:
                    out |= ~self.eligible[y.long()]
                if predicate is not None:
                    out |= self._fails_predicate(y, parts)
                filtered += (out & take[lo:hi]).sum()
        try:
            res = Metrics.catalogue_metrics(slot, rank, ks, take)
        except ValueError as e:
            raise ValueError(f"{what}: the dataset holds no +1 pair") from e
        if filtering:
            res["filtered_targets"] = int(filtered)
        return res

    def recommend(self, query_id, num_recommendations: int = 10) -> Dict[str, Any]:
        """Generate complementary product recommendations (inference.py:64-124): same result dict."""
        q = torch.tensor([self._to_index(query_id)], dtype=torch.int32)
        types, idx, sc = self.recommend_batch(q, num_recommendations)
        types, idx, sc = types[0].cpu().numpy(), idx[0].cpu().numpy(), sc[0].cpu().numpy()
        recommendations, scores = [], []
        for j in range(len(types)):
            keep = idx[j] >= 0
            if not keep.any():
                continue                                                          # `if not type_products: continue`
            ids = idx[j][keep]
            recommendations.append([self.product_ids[i] for i in ids] if self.product_ids is not None else ids.tolist())
            scores.append(sc[j][keep])
        return {"complementary_types": types.tolist(), "recommendations": recommendations, "scores": scores}


class CompactInference(PCompanionInference):
    """PCompanionInference over an ops.CompactCatalogue that also RANKS from the bf16 copy: rank_targets and evaluate_catalogue
    go through ops.rank_grouped_bf16 (pc_rank_grouped_bf16), whose (row, product) scores are the bits recommend_batch's
    entries order by -- pc_retrieve_topk_grouped_bf16 up to 16, pc_retrieve_list_grouped_bf16 up to 256.  So rank < n exactly
    when recommend_batch(q, n) of this object holds the target at that position, evaluate_catalogue's hit@k for k <= 256
    describes recommend_batch(q, k) exactly, and both are measured over the ROUNDED table that is served.  No fp32 features are read by this object, and a DeviceBPG generated
    without them is accepted: recommend_batch and rank_targets (folded by Metrics.catalogue_metrics over the caller's own pairs)
    run on such a graph.  evaluate_catalogue takes a ComplementaryIndexDataset over the SAME graph object, and that dataset
    refuses a DeviceBPG without features: over a device graph it runs only while the graph still holds them.
    set_exclusions / set_eligible work as in the parent.
    A class of its own: PCompanionInference keeps refusing ranks with any bf16 catalogue."""

    def __init__(self, model, config, bpg, product_ids=None, catalogue=None):
        if not isinstance(catalogue, ops.CompactCatalogue):
            raise ValueError(f"CompactInference: catalogue must be an ops.CompactCatalogue, got "
                             f"{type(catalogue).__name__}; PCompanionInference serves the other catalogues")
        super().__init__(model, config, bpg, product_ids, catalogue=catalogue)

    def _rank_guard(self, what):
        pass

    def _rank_entry(self):
        return ops.rank_grouped_bf16, self.catalogue


class SimilarProducts(_CandidateFilters):
    """Substitutes: the nearest products of a query under Euclidean distance over an embedding table -- the order Product2Vec's
    triplet loss trains for.  |q - e_p|^2 = |q|^2 - 2 (<q, e_p> - |e_p|^2 / 2), so the nearest product is the largest
    <q, e_p> + b_p with b_p = -|e_p|^2 / 2: ops.retrieve_topk_grouped / ops.rank_grouped with bias = ops.half_sq_norm_bias(table),
    formed once here.  Everything around the grouped retrieval carries over: the plan, the slices, the total order (score
    descending, product index ascending), exclusion lists, "rank < n exactly when the list holds the target at position rank",
    bitwise determinism.

    table: a [P, D] fp32 device tensor, D 128 or 256 -- Product2Vec.generate_embedding_table's export, or the raw features.
    bpg: an IntBPG or a world-1 DeviceBPG over the same P products (type_idx).
    scope "type": the candidates of a query are the products of its own type (ops.type_csr); "catalogue": every product, as
    one type (rowptr = [0, P], col = arange(P)).
    By default the query itself is excluded (set_exclusions() over an empty CSR with include_self), so a product is never its
    own neighbour; the co-view graph is NOT excluded -- co-viewed products are the substitutes being looked for.
    set_exclusions(False) removes the set; set_eligible(mask) serves and ranks over the eligible products only.
    similar_batch / similar_capped_batch serve up to MAX_N = 16 (the 16-entry biased retrieval), similar_list_batch /
    similar_capped_list_batch up to MAX_LIST = 256 (ops.retrieve_list_grouped_biased): the same score bits and order."""

    MAX_N = 16

    def __init__(self, table, bpg, scope="type"):
        if scope not in ("type", "catalogue"):
            raise ValueError(f"SimilarProducts: scope must be 'type' or 'catalogue', got {scope!r}")
        table = self._check_table(table)
        if isinstance(bpg, DeviceBPG) and bpg.world != 1:
            raise ValueError(f"SimilarProducts: this DeviceBPG holds a cyclic 1/{bpg.world} shard (rank {bpg.rank}); serving "
                             "needs the whole catalogue on one device -- generate it with world = 1")
        if bpg.num_products != table.shape[0]:
            raise ValueError(f"SimilarProducts: the table holds {table.shape[0]} rows, the graph {bpg.num_products} products")
        self.table, self.bpg, self.scope, self.device = table, bpg, scope, table.device
        self._graph = bpg.cuda(self.device)
        self.type_idx = self._graph["type_idx"]
        p = table.shape[0]
        if scope == "type":
            self._scope_type, self._scope_types = self.type_idx, bpg.n_types
            self._all_products = ops.type_csr(self.type_idx, bpg.n_types)
        else:
            self._scope_type, self._scope_types = torch.zeros(p, dtype=torch.int32, device=self.device), 1
            self._all_products = (torch.tensor([0, p], dtype=torch.int32, device=self.device),
                                  torch.arange(p, dtype=torch.int32, device=self.device))
        self.type_rowptr, self.type_col = self._all_products
        self.cand_type, self.eligible, self.exclusions = self._scope_type, None, None
        self.bias = self._half_sq_norm()                  # once per catalogue
        self.set_exclusions()                             # the query itself

    # What differs between the tables (CompactSimilarProducts: the bf16 copy) is behind these hooks: the check of the table,
    # the bias, the three device calls (retrieval up to 16, list, rank) and the gather of fp32 rows.
    def _check_table(self, table):
        if not torch.is_tensor(table) or table.dtype != torch.float32:
            raise ValueError(f"SimilarProducts: the table must be a [P, D] float32 device tensor, got "
                             f"{table.dtype if torch.is_tensor(table) else type(table).__name__}")
        if table.dim() != 2 or table.shape[1] not in (128, 256) or table.shape[0] < 1:
            raise ValueError(f"SimilarProducts: the table must be [P, 128 or 256], got {tuple(table.shape)}")
        if not table.is_cuda or not table.is_contiguous():
            raise ValueError("SimilarProducts: the table must be a contiguous device tensor")
        return table

    def _half_sq_norm(self):
        return ops.half_sq_norm_bias(self.table)

    def _retrieve(self, q, row_type, n, exclude):
        return ops.retrieve_topk_grouped(q, row_type, self.type_rowptr, self.type_col, self.table, n, exclude=exclude,
                                         bias=self.bias)

    def _retrieve_list(self, q, row_type, n, exclude):
        return ops.retrieve_list_grouped_biased(q, row_type, self.type_rowptr, self.type_col, self.table, self.bias, n,
                                                exclude=exclude)

    def _rank(self, q, row_type, target_idx, **lists):
        return ops.rank_grouped(q, row_type, target_idx, self.type_rowptr, self.type_col, self.table, bias=self.bias, **lists)

    def _rows(self, ids):
        """[..., D] fp32: the rows `ids` (int64) of the table"""
        return self.table[ids]

    def _candidate_types(self):
        return self._scope_type, self._scope_types

    def _default_exclusions(self):
        p = int(self.type_idx.shape[0])
        return (torch.zeros(p + 1, dtype=torch.int32, device=self.device), torch.zeros(0, dtype=torch.int32, device=self.device))

    @torch.no_grad()
    def similar_batch(self, query_idx: torch.Tensor, n: int = 10):
        """The n nearest candidates of every query, nearest first: (idx [B, n] int32, -1 past the end; dist [B, n] fp32, +inf
        past the end).  The order is the biased retrieval's; dist is recomputed for the returned ids as |q - e + 1e-6|_2, the
        distance of the triplet loss (F.pairwise_distance) -- not derived from the score, whose terms cancel."""
        n = self._neighbours(n)
        query_idx = self._queries("similar_batch", query_idx)
        if query_idx.shape[0] == 0:
            return self._no_neighbours(n)
        q = self._rows(query_idx.long())
        idx, _ = self._retrieve(q, self._scope_type[query_idx.long()].contiguous(), n, self._exclude_rows(query_idx))
        return idx, self._distances(q, idx)

    @torch.no_grad()
    def similar_capped_batch(self, query_idx: torch.Tensor, n: int = 10, group: torch.Tensor = None, cap: int = 1,
                             own_group: bool = False):
        """similar_batch with at most `cap` products of one product group per list, and -- unless own_group -- none of the
        query's own group: a product's nearest neighbours are its own variants, and they are not its substitutes.  group [P]
        int32 on the device, negative = ungrouped (never capped, never banned); None: nothing is grouped.  The pool is this
        object's similar_batch(query_idx, MAX_N): its 16 nearest candidates with their reported distances.  ops.cap_lists runs on
        the NEGATED distances, so nearer is better and equal distances go to the lower product index, with
        row_ban = group[query_idx] unless own_group.  Returns (idx [B, n] int32, dist [B, n] fp32), the distances those
        similar_batch reported for the same ids, -1 / +inf past the end.  1 <= n <= 16.
        THE LIMIT: the pool is 16 products, because this method's pool is the 16-entry biased retrieval's.  In a heavily
        varianted neighbourhood most of the 16 are the query's own variants or share a few groups, and the list comes back SHORT
        (even empty) although the catalogue holds further neighbours.  similar_capped_list_batch is the same rule over a pool of
        up to MAX_LIST = 256 candidates (the biased long-list entry, ops.retrieve_list_grouped_biased): use it where the
        neighbourhoods are varianted."""
        n = int(n)
        if not 1 <= n <= self.MAX_N:
            raise ValueError(f"similar_capped_batch: 1 to {self.MAX_N} neighbours per query, got {n}")
        return self._capped("similar_capped_batch", self.similar_batch, query_idx, n, group, cap, own_group, self.MAX_N)

    def _capped(self, what, pool_of, query_idx, n, group, cap, own_group, pool):
        """The group cap's rule on the `pool` nearest candidates that pool_of(query_idx, pool) serves (similar_capped_batch)."""
        cap = _check_group(what, group, cap)
        self._group_covers(what, group)
        query_idx = self._queries(what, query_idx)
        if query_idx.shape[0] == 0:
            return self._no_neighbours(n)
        idx, dist = pool_of(query_idx, pool)
        ban = group[query_idx.long()].contiguous() if group is not None and not own_group else None
        idx, near = ops.cap_lists(idx, -dist, n, group, cap, row_ban=ban)
        return idx, -near

    MAX_LIST = 256                    # ops.RETRIEVE_LIST_MAX_N: what the biased long-list entry serves
    DIST_BYTES = 64 << 20             # similar_list_batch: the bytes of ONE [queries, n, D] fp32 temporary of the distances

    @torch.no_grad()
    def similar_list_batch(self, query_idx: torch.Tensor, n: int = 64):
        """similar_batch's contract for 1 <= n <= MAX_LIST = 256: (idx [B, n] int32, -1 past the end; dist [B, n] fp32, +inf
        past the end), nearest first, through ops.retrieve_list_grouped_biased -- the same score bits and total order, so for
        n <= 16 ids and distances are similar_batch's bit for bit.  The distances are recomputed as there, over chunks of
        DIST_BYTES / (4 n D) queries: the gathered rows [B, n, D] and their differences are 0.5 GB each at B = 4096, n = 256,
        D = 128 unchunked, and at most DIST_BYTES = 64 MiB each here; a row's distance does not depend on its chunk."""
        n = self._list_length("similar_list_batch", n)
        query_idx = self._queries("similar_list_batch", query_idx)
        if query_idx.shape[0] == 0:
            return self._no_neighbours(n)
        q = self._rows(query_idx.long())
        idx, _ = self._retrieve_list(q, self._scope_type[query_idx.long()].contiguous(), n, self._exclude_rows(query_idx))
        return idx, self._list_distances(q, idx)

    @torch.no_grad()
    def similar_where_batch(self, query_idx: torch.Tensor, n: int = 10, lo: torch.Tensor = None, hi: torch.Tensor = None,
                            need: torch.Tensor = None, deny: torch.Tensor = None):
        """similar_list_batch's contract (1 <= n <= MAX_LIST; idx [B, n] int32, dist [B, n] fp32, -1 / +inf past the end) over
        the candidates that pass a per-query predicate on the installed attributes (set_attributes): lo / hi [B] float32 a band
        on value[p] (band_around: substitutes around the query's price; hi = value[q]: cheaper ones), need / deny [B] int32
        masks on flags[p].  ops.retrieve_list_grouped_where under this object's bias, in both scopes: what similar_list_batch
        serves under set_eligible(mask of the predicate), ids and distances bit for bit, for predicates that differ per query.
        ValueError before anything is computed where no attributes are installed or none of the four is given."""
        n = self._list_length("similar_where_batch", n)
        where = self._row_predicate("similar_where_batch", int(query_idx.shape[0]) if query_idx.dim() else -1, lo, hi, need, deny)
        query_idx = self._queries("similar_where_batch", query_idx)
        if query_idx.shape[0] == 0:
            return self._no_neighbours(n)
        q = self._rows(query_idx.long())
        idx, _ = ops.retrieve_list_grouped_where(q, self._scope_type[query_idx.long()].contiguous(), self.type_rowptr,
                                                 self.type_col, self.table, n, where, exclude=self._exclude_rows(query_idx),
                                                 bias=self.bias)
        return idx, self._list_distances(q, idx)

    @torch.no_grad()
    def similar_capped_list_batch(self, query_idx: torch.Tensor, n: int = 10, group: torch.Tensor = None, cap: int = 1,
                                  own_group: bool = False, pool: int = 64):
        """similar_capped_batch's rule over a longer pool: ops.cap_lists on the negated reported distances of this object's
        similar_list_batch(query_idx, pool), row_ban = group[query_idx] unless own_group.  1 <= n <= pool <= MAX_LIST = 256.
        Returns (idx [B, n] int32, dist [B, n] fp32), -1 / +inf past the end: a list is short only where the pool itself holds
        fewer than n products that the cap lets through."""
        n, pool = int(n), int(pool)
        if not 1 <= n <= pool <= self.MAX_LIST:
            raise ValueError(f"similar_capped_list_batch: 1 <= n <= pool <= {self.MAX_LIST} neighbours per query, got n = {n}, "
                             f"pool = {pool}")
        return self._capped("similar_capped_list_batch", self.similar_list_batch, query_idx, n, group, cap, own_group, pool)

    def _list_length(self, what, n):
        """n of similar_list_batch as an int; outside 1 .. MAX_LIST: ValueError, before anything of the object is read."""
        n = int(n)
        if not 1 <= n <= self.MAX_LIST:
            raise ValueError(f"{what}: 1 to {self.MAX_LIST} neighbours per query, got {n}")
        return n

    def _list_distances(self, q, idx):
        """_distances over chunks of queries whose [rows, n, D] fp32 temporaries hold at most DIST_BYTES each."""
        rows = max(1, self.DIST_BYTES // (4 * idx.shape[1] * q.shape[1]))
        if q.shape[0] <= rows:
            return self._distances(q, idx)
        return torch.cat([self._distances(q[lo:lo + rows], idx[lo:lo + rows]) for lo in range(0, q.shape[0], rows)])

    def _neighbours(self, n):
        """n of similar_batch as an int; outside 1 .. MAX_N: ValueError, before anything of the object is read."""
        n = int(n)
        if not 1 <= n <= self.MAX_N:
            raise ValueError(f"similar_batch: 1 to {self.MAX_N} neighbours per query, got {n}")
        return n

    def _queries(self, what, query_idx):
        query_idx = query_idx.to(self.device).to(torch.int32).contiguous()
        if query_idx.dim() != 1:
            raise ValueError(f"{what}: query_idx must be 1-D")
        return query_idx

    def _no_neighbours(self, n):
        """similar_batch of no query"""
        return (torch.empty(0, n, dtype=torch.int32, device=self.device), torch.empty(0, n, dtype=torch.float32, device=self.device))

    def _distances(self, q, idx):
        """[B, n] fp32: |q[b] - table[idx[b, j]] + 1e-6|_2, +inf where idx is -1"""
        e = self._rows(idx.clamp(min=0).long())                                   # [B, n, D]
        dist = (q[:, None, :] - e + 1e-6).norm(dim=2)
        return torch.where(idx >= 0, dist, torch.full_like(dist, float("inf")))

    @torch.no_grad()
    def rank_pairs(self, anchor_idx: torch.Tensor, target_idx: torch.Tensor):
        """Where does target_idx[b] stand among the neighbours of anchor_idx[b]?  slot[b] = 0 where the target is a candidate
        of the anchor's scope (its type under scope "type"; eligible), -1 otherwise; rank[b] = the target's position in
        similar_batch's list, were the list the whole scope -- rank < n exactly when similar_batch(anchor, n) holds the target
        at that position -- and -1 as ops.rank_grouped defines: no candidate of the scope, in the anchor's exclusion list (the
        anchor itself by default), outside the catalogue.  (slot, rank) int32 [B] on the device; nothing is read back."""
        return self._rank_pairs("rank_pairs", anchor_idx, target_idx)

    def _rank_where(self, q, row_type, target_idx, where, **lists):
        return ops.rank_grouped_where(q, row_type, target_idx, self.type_rowptr, self.type_col, self.table, where, bias=self.bias,
                                      **lists)

    def _rank_pairs(self, what, anchor_idx, target_idx, where=None):
        """rank_pairs; with an ops.RowWhere rank_pairs_where (ops.rank_grouped_where in _rank's place)"""
        rank_rows = self._rank if where is None else (lambda *rows, **lists: self._rank_where(*rows, where, **lists))
        anchor_idx = anchor_idx.to(self.device).to(torch.int32).contiguous()
        target_idx = target_idx.to(self.device).to(torch.int32).contiguous()
        if anchor_idx.dim() != 1 or anchor_idx.shape != target_idx.shape:
            raise ValueError(f"{what}: anchor_idx and target_idx must be 1-D and of equal length")
        if anchor_idx.shape[0] == 0:
            e = torch.empty(0, dtype=torch.int32, device=self.device)
            return e, e.clone()
        p = self.table.shape[0]
        row_type = self._scope_type[anchor_idx.long()]
        inside = (target_idx >= 0) & (target_idx < p)
        candidate = inside & (self.cand_type[target_idx.long().clamp(0, p - 1)] == row_type)
        slot = torch.where(candidate, 0, -1).to(torch.int32)
        q = self._rows(anchor_idx.long())
        exclude = self._exclude_rows(anchor_idx)
        if exclude is not None:
            rank, _ = rank_rows(q, row_type.contiguous(), target_idx, exclude=exclude, cand_type=self.cand_type)
            return slot, rank
        # no lists: a target that is no candidate costs no search
        row_type = torch.where(candidate, row_type, torch.full_like(row_type, -1)).contiguous()
        rank, _ = rank_rows(q, row_type, target_idx)
        return slot, rank

    @torch.no_grad()
    def rank_pairs_where(self, anchor_idx: torch.Tensor, target_idx: torch.Tensor, lo: torch.Tensor = None,
                         hi: torch.Tensor = None, need: torch.Tensor = None, deny: torch.Tensor = None):
        """rank_pairs under a per-anchor predicate on the installed attributes (set_attributes; lo / hi / need / deny [B] as in
        similar_where_batch): rank[b] = the number of candidates of the anchor's scope that PASS anchor b's predicate and stand
        in front of the target -- rank < n exactly when similar_where_batch(anchor, n, ...) holds the target at that position
        -- under this object's bias, scope, exclusions and eligibility; -1 as in rank_pairs and where the target fails its own
        anchor's predicate (its slot stays).  One call of ops.rank_grouped_where, the entry by the table's dtype.  (slot, rank)
        int32 [B] on the device.  ValueError before anything is computed where no attributes are installed or none of the
        four is given."""
        where = self._row_predicate("rank_pairs_where", int(anchor_idx.shape[0]) if anchor_idx.dim() else -1, lo, hi, need, deny)
        return self._rank_pairs("rank_pairs_where", anchor_idx, target_idx, where)

    def evaluate_pairs_where(self, pairs, predicate, ks=(1, 3, 10, 100), chunk: int = 65536) -> Dict[str, Any]:
        """evaluate_pairs of what similar_where_batch serves: predicate(anchor_idx) -- an int32 device vector, a chunk's
        anchors -- returns a dict with any of lo, hi, need, deny ([chunk] tensors); the chunks go through rank_pairs_where.
        Returns evaluate_pairs' dict; a pair whose target fails its own anchor's predicate is a miss."""
        what = "evaluate_pairs_where"
        if self.attributes is None:
            raise ValueError(f"{what}: no per-product attributes are installed (set_attributes)")
        if not callable(predicate):
            raise ValueError(f"{what}: predicate must be a callable of the chunk's anchor ids, got {type(predicate).__name__}")
        return self._evaluate_pairs(what, pairs, ks, chunk, predicate)

    def evaluate_pairs(self, pairs, ks=(1, 3, 10, 100), chunk: int = 65536) -> Dict[str, Any]:
        """Are held-out similar pairs among the neighbours that are served?  pairs [M, 2] (anchor, target) int -- whatever the
        caller held out, e.g. the co-view pairs of a later window of edges.  Chunks of `chunk` pairs go through rank_pairs
        into two device vectors; Metrics.catalogue_metrics folds them and reads back once: {"pairs", "type_hit" (the share
        whose target is a candidate of the anchor's scope), "hit@k" for k in ks, "mrr", "median_rank"}."""
        return self._evaluate_pairs("evaluate_pairs", pairs, ks, chunk)

    def _evaluate_pairs(self, what, pairs, ks, chunk, predicate=None):
        """evaluate_pairs; with a predicate evaluate_pairs_where (the chunks through rank_pairs_where)"""
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"{what}: chunk must be positive")
        if not torch.is_tensor(pairs):
            pairs = torch.from_numpy(np.ascontiguousarray(np.asarray(pairs), dtype=np.int32))
        if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] == 0:
            raise ValueError(f"{what}: expected a non-empty [M, 2] array of (anchor, target), got {tuple(pairs.shape)}")
        pairs = pairs.to(self.device).to(torch.int32)
        m = pairs.shape[0]
        slot = torch.empty(m, dtype=torch.int32, device=self.device)
        rank = torch.empty(m, dtype=torch.int32, device=self.device)
        for lo in range(0, m, chunk):
            hi = min(lo + chunk, m)
            if predicate is None:
                slot[lo:hi], rank[lo:hi] = self.rank_pairs(pairs[lo:hi, 0], pairs[lo:hi, 1])
            else:
                parts = predicate(pairs[lo:hi, 0].contiguous())
                if not isinstance(parts, dict) or not set(parts) <= {"lo", "hi", "need", "deny"}:
                    raise ValueError(f"{what}: predicate(anchor_idx) must return a dict with any of lo, hi, need, deny, got "
                                     f"{sorted(parts) if isinstance(parts, dict) else type(parts).__name__}")
                slot[lo:hi], rank[lo:hi] = self.rank_pairs_where(pairs[lo:hi, 0], pairs[lo:hi, 1], **parts)
        return Metrics.catalogue_metrics(slot, rank, ks)


class CompactSimilarProducts(SimilarProducts):
    """SimilarProducts over the bf16 copy of the table alone: substitutes by Euclidean distance to the STORED (rounded) rows,
    for a deployment that gave the fp32 table back.  catalogue: an ops.CompactCatalogue, or a contiguous [P, 128 | 256]
    torch.bfloat16 device tensor (wrapped in one).  The same scopes, default self-exclusion, set_exclusions / set_eligible,
    MAX_N and MAX_LIST, and the same methods:
      similar_batch, similar_list_batch, similar_capped_batch, similar_capped_list_batch  all through the biased bf16 list
                  entry (ops.retrieve_list_grouped_bf16_biased), at n <= 16 too, with bias = the catalogue's .half_sq_norm;
      rank_pairs / evaluate_pairs  through ops.rank_grouped_bf16(bias=): rank < n exactly when similar_list_batch(anchor, n)
                  holds the target at that position.
    The query row is the stored row widened (exactly) to fp32; the reported distances are |q - e + 1e-6|_2 over widened
    gathered rows, in chunks of DIST_BYTES.  An fp32 table is never materialised: the widened rows are the [B, D] queries and
    the [rows, n, D] chunks of the distances alone.  On a table that bf16 represents exactly AND whose partial sums are exact in
    both score chains (small integers) every method returns what SimilarProducts(table.float()) returns, bit for bit; on merely
    representable data the two chains' different summation orders may order a near-tie differently."""

    def _check_table(self, catalogue):
        if torch.is_tensor(catalogue):
            if catalogue.dtype != torch.bfloat16:
                raise ValueError(f"CompactSimilarProducts: a table tensor must be torch.bfloat16 (ops.catalogue_bf16), got "
                                 f"{catalogue.dtype}; SimilarProducts serves the float32 table")
            catalogue = ops.CompactCatalogue(catalogue)   # (its shape, device and layout checks)
        if not isinstance(catalogue, ops.CompactCatalogue):
            raise ValueError(f"CompactSimilarProducts: the catalogue must be an ops.CompactCatalogue or a [P, 128 or 256] "
                             f"bfloat16 device tensor, got {type(catalogue).__name__}")
        self.compact = catalogue
        return catalogue.table

    def _half_sq_norm(self):
        return self.compact.half_sq_norm

    def _retrieve(self, q, row_type, n, exclude):
        return self._retrieve_list(q, row_type, n, exclude)

    def _retrieve_list(self, q, row_type, n, exclude):
        return ops.retrieve_list_grouped_bf16_biased(q, row_type, self.type_rowptr, self.type_col, self.table, self.bias, n,
                                                     exclude=exclude)

    def _rank(self, q, row_type, target_idx, **lists):
        return ops.rank_grouped_bf16(q, row_type, target_idx, self.type_rowptr, self.type_col, self.table, bias=self.bias,
                                     **lists)

    def _rows(self, ids):
        return self.table[ids].float()                    # (the gathered rows alone are widened)


class IndexedSimilarProducts(SimilarProducts):
    """SimilarProducts(scope="catalogue") served through a k-means cell index (ops.build_cell_index): a query is scored against
    the products of its nprobe nearest cells, not against the catalogue.  similar_batch is APPROXIMATE in one way only: a
    neighbour outside the probed cells is missed.  Inside them everything is the parent's -- the score bits, the total order
    (score descending, product index ascending), exclusions, eligibility -- so the list is exactly the parent's order
    restricted to the probed cells' products, and with nprobe == n_cells it is the parent's list bit for bit.
    rank_pairs / evaluate_pairs are the parent's exact whole-catalogue code: an approximate rank has no meaning.

    index: a CellIndex over this table; or n_cells (with iters, seed) to build one here.  nprobe: the default number of cells
    a query probes, 1 .. min(16, n_cells)."""

    MAX_NPROBE = 16

    def __init__(self, table, bpg, index=None, n_cells=None, nprobe=8, iters=10, seed=0):
        name = type(self).__name__
        if (index is None) == (n_cells is None):
            raise ValueError(f"{name}: pass an index, or n_cells to build one (not both)")
        rows = table.table if isinstance(table, ops.CompactCatalogue) else table
        if index is not None and torch.is_tensor(rows) and rows.dim() == 2 \
                and (index.num_products, index.dim) != tuple(rows.shape):
            raise ValueError(f"{name}: the index is over [{index.num_products}, {index.dim}], the table is {tuple(rows.shape)}")
        cells = int(n_cells) if index is None else int(index.n_cells)
        self._check_nprobe(name, nprobe, cells)
        super().__init__(table, bpg, scope="catalogue")
        if index is None:
            index = self._build_index(cells, iters, seed)
        self.index, self.n_cells, self.nprobe = index, cells, int(nprobe)
        self.cell_rowptr, self.cell_col = index.cell_rowptr, index.cell_col
        self._one_cell_type = (torch.tensor([0, cells], dtype=torch.int32, device=self.device),
                               torch.arange(cells, dtype=torch.int32, device=self.device))

    # What differs over the bf16 copy (IndexedCompactSimilarProducts) beyond the parent's hooks: the index build and the scan of
    # the probed cells.
    def _build_index(self, n_cells, iters, seed):
        return ops.build_cell_index(self.table, n_cells, iters=iters, seed=seed)

    def _scan(self, rows, cells, n, exclude, long):
        """The grouped retrieval over the B nprobe rows, a probed cell in the place of a type."""
        if long:
            return ops.retrieve_list_grouped_biased(rows, cells, self.cell_rowptr, self.cell_col, self.table, self.bias, n,
                                                    exclude=exclude)
        return ops.retrieve_topk_grouped(rows, cells, self.cell_rowptr, self.cell_col, self.table, n, exclude=exclude,
                                         bias=self.bias)

    @classmethod
    def _check_nprobe(cls, what, nprobe, n_cells):
        top = min(cls.MAX_NPROBE, n_cells)
        if not 1 <= int(nprobe) <= top:
            raise ValueError(f"{what}: nprobe must be in [1, min({cls.MAX_NPROBE}, n_cells) = {top}], got {nprobe}")
        return int(nprobe)

    def set_eligible(self, mask=None):
        """The parent's filter for the exact paths (the one-type CSR and cand_type), and the cell CSR filtered the same way:
        type_csr of the eligible products' cells."""
        super().set_eligible(mask)
        if self.eligible is None:
            self.cell_rowptr, self.cell_col = self.index.cell_rowptr, self.index.cell_col
            return self
        ids = torch.nonzero(self.eligible).reshape(-1).to(torch.int32)
        rowptr, local = ops.type_csr(self.index.cell_of[ids.long()].contiguous(), self.n_cells)
        self.cell_rowptr, self.cell_col = rowptr, ids[local.long()].contiguous()
        return self

    def _probe(self, q, nprobe):
        rowptr, col = self._one_cell_type
        zeros = torch.zeros(q.shape[0], dtype=torch.int32, device=self.device)
        if nprobe > self.MAX_N:                           # (above the 16-entry kernel: the same total order, the long-list entry)
            cells, _ = ops.retrieve_list_grouped_biased(q, zeros, rowptr, col, self.index.centroids, self.index.centroid_bias,
                                                        nprobe)
            return cells
        cells, _ = ops.retrieve_topk_grouped(q, zeros, rowptr, col, self.index.centroids, nprobe, bias=self.index.centroid_bias)
        return cells

    def _search(self, query_idx, q, n, nprobe, long=False):
        """(idx [B, n] int32, score [B, n] fp32 = the biased retrieval's own score bits; -1 / -inf past the end) of the checked
        queries query_idx [B] int32 with rows q [B, D]: steps 1 to 3 of similar_batch; long: of similar_list_batch (step 2
        through the biased long-list entry, n up to MAX_LIST)."""
        b = q.shape[0]
        cells = self._probe(q, nprobe)                                            # [B, nprobe]
        rows = q.repeat_interleave(nprobe, dim=0)                                 # [B nprobe, D]
        exclude = self._exclude_rows(query_idx, nprobe)
        idx, score = self._scan(rows, cells.reshape(-1), n, exclude, long)
        return ops.merge_lists(idx.view(b, nprobe, n), score.view(b, nprobe, n))

    @torch.no_grad()
    def probe_cells(self, query_idx: torch.Tensor, nprobe: int = None):
        """[B, nprobe] int32: the nprobe nearest cells of every query, nearest first (the biased 16-entry retrieval over the
        centroids; ties to the lower cell)."""
        nprobe = self._check_nprobe("probe_cells", self.nprobe if nprobe is None else nprobe, self.n_cells)
        query_idx = self._queries("probe_cells", query_idx)
        if query_idx.shape[0] == 0:
            return torch.empty(0, nprobe, dtype=torch.int32, device=self.device)
        return self._probe(self._rows(query_idx.long()), nprobe)

    @torch.no_grad()
    def similar_batch(self, query_idx: torch.Tensor, n: int = 10, nprobe: int = None):
        """The parent's contract over the non-excluded, eligible products of each query's nprobe nearest cells (None: the
        constructor's): (idx [B, n] int32, -1 past the end; dist [B, n] fp32, +inf past the end).  Four steps: probe the
        centroids; one grouped retrieval over B nprobe rows (row type = the probed cell, row key = the query); merge_lists of a
        query's nprobe lists; the distances recomputed as the parent does."""
        n = self._neighbours(n)
        nprobe = self._check_nprobe("similar_batch", self.nprobe if nprobe is None else nprobe, self.n_cells)
        query_idx = self._queries("similar_batch", query_idx)
        if query_idx.shape[0] == 0:
            return self._no_neighbours(n)
        q = self._rows(query_idx.long())
        idx, _ = self._search(query_idx, q, n, nprobe)
        return idx, self._distances(q, idx)

    @torch.no_grad()
    def similar_list_batch(self, query_idx: torch.Tensor, n: int = 64, nprobe: int = None):
        """similar_batch's four steps for 1 <= n <= MAX_LIST = 256, the grouped retrieval over the B nprobe rows through the
        biased long-list entry (ops.merge_lists takes lists of up to 256): the parent's similar_list_batch restricted to the
        probed cells' products, and with nprobe == n_cells that list bit for bit.  The distances are the parent's, chunked."""
        n = self._list_length("similar_list_batch", n)
        nprobe = self._check_nprobe("similar_list_batch", self.nprobe if nprobe is None else nprobe, self.n_cells)
        query_idx = self._queries("similar_list_batch", query_idx)
        if query_idx.shape[0] == 0:
            return self._no_neighbours(n)
        q = self._rows(query_idx.long())
        idx, _ = self._search(query_idx, q, n, nprobe, long=True)
        return idx, self._list_distances(q, idx)

    def similar_where_batch(self, query_idx, n=10, lo=None, hi=None, need=None, deny=None):
        """Not served through the cell index: the per-query attribute filter is the exact classes'."""
        raise NotImplementedError(f"{type(self).__name__}.similar_where_batch: the per-query attribute filter is not served "
                                  "through the cell index; SimilarProducts / CompactSimilarProducts serve it")

    @torch.no_grad()
    def recall(self, query_idx: torch.Tensor, n: int = 10, nprobe: int = None):
        """A device scalar (fp32): the share of the ids of the exact lists (SimilarProducts.similar_batch on this object) that
        the indexed lists of the same queries hold; 1 where the exact lists are empty."""
        nprobe = self._check_nprobe("recall", self.nprobe if nprobe is None else nprobe, self.n_cells)
        exact, _ = SimilarProducts.similar_batch(self, query_idx, n)
        got, _ = self.similar_batch(query_idx, n, nprobe)
        held = ((exact[:, :, None] == got[:, None, :]) & (exact[:, :, None] >= 0)).any(dim=2).sum()
        total = (exact >= 0).sum()
        return torch.where(total > 0, held.float() / total.clamp(min=1).float(), torch.ones((), device=self.device))


class IndexedCompactSimilarProducts(IndexedSimilarProducts, CompactSimilarProducts):
    """CompactSimilarProducts(scope="catalogue") served through a k-means cell index, from the bf16 copy of the catalogue alone:
    IndexedSimilarProducts' four steps for a deployment that gave the fp32 table back.  catalogue: an ops.CompactCatalogue or a
    contiguous [P, 128 | 256] torch.bfloat16 device tensor.  index: a CellIndex over these P products and D -- from
    ops.build_cell_index_bf16, or from ops.build_cell_index on the fp32 table before it was given back --; or n_cells (with
    iters, seed) to build one here through ops.build_cell_index_bf16.  nprobe: 1 .. min(MAX_NPROBE = 64, n_cells).
      probe       the query row is the stored row widened (exactly) to fp32; the probe runs over the fp32 centroids with the fp32
                  biased entries: for nprobe <= 16 the 16-entry retrieval (IndexedSimilarProducts.probe_cells' bits for the same
                  index and rows), for 17 <= nprobe <= 64 ops.retrieve_list_grouped_biased -- the same total order, so the
                  first 16 columns agree;
      scan        ops.retrieve_list_grouped_bf16_biased over the cell CSR at every n, bias = the catalogue's .half_sq_norm: a
                  (row, product) score comes from the kernel and chain of CompactSimilarProducts;
      merge       ops.merge_lists (up to 64 lists of up to 256);
      distances   the compact parent's, over widened gathered rows, chunked.
    The cells partition the products and every selection is under (score descending, index ascending): the served list is the
    exact compact list restricted to the non-excluded, eligible products of the probed cells, and with nprobe == n_cells that
    list bit for bit, ids and distances.  similar_batch (n <= 16), similar_list_batch (n <= 256), the capped methods,
    probe_cells, set_eligible and similar_where_batch (NotImplementedError) are IndexedSimilarProducts'; recall is relative
    to the exact list over the ROUNDED rows; rank_pairs / evaluate_pairs are the exact inherited ones (ops.rank_grouped_bf16).
    An fp32 table is never materialised."""

    MAX_NPROBE = 64                   # ops.MERGE_MAX_LISTS: what merge_lists takes; the probe above 16 is the long-list entry

    def _build_index(self, n_cells, iters, seed):
        return ops.build_cell_index_bf16(self.compact, n_cells, iters=iters, seed=seed)

    def _scan(self, rows, cells, n, exclude, long):
        return ops.retrieve_list_grouped_bf16_biased(rows, cells, self.cell_rowptr, self.cell_col, self.table, self.bias, n,
                                                     exclude=exclude)
