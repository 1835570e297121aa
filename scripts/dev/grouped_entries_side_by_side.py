#!/usr/bin/env python3
"""Two builds of libpcompanion_hip.so side by side, no device involved: every workspace query of the type-grouped catalogue
entries over a grid of (rows, n_types, n, slices) with each bound and one step past it, and the return code of refused calls
of those entries -- the cases of the family's error-code tests (tests/test_gpu_retrieval_grouped.py, test_gpu_exclusions.py,
test_gpu_retrieval_list.py, test_gpu_retrieval_bf16.py, test_gpu_compact_catalogue.py, test_gpu_nearest.py, test_gpu_rank_grouped.py, test_gpu_rank_bf16.py, test_gpu_where_rank.py and the *_host.py ones)
and around them every single null pointer, every pair of two changed arguments out of the edge values below, and every
combination of present / absent exclusion arguments, a bf16 table off its 16-byte alignment, and for the entries under a
predicate every present / absent shape of the pc_row_where.  No call here can launch: the workspace handed in is one byte short at
the most, and the pointers are never dereferenced before that check.

    python scripts/dev/grouped_entries_side_by_side.py PARENT.so CHILD.so

Exit status 1 when anything differs, or when the parent does not refuse a call."""
import collections
import ctypes
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from p_companion_amd import _lib                                        # noqa: E402

ROWS = (-1, 0, 1, 2, 15, 16, 17, 63, 64, 65, 4096, 100_000)
TYPES = (-1, 0, 1, 2, 100, 1024, 1025, 34_800)
NS = (-1, 0, 1, 2, 15, 16, 17, 32, 33, 96, 97, 255, 256, 257)
SLICES = (-1, 0, 1, 15, 16, 17, 63, 64, 65)
TOPN = ("pc_retrieve_topk_grouped", "pc_retrieve_topk_grouped_excluding", "pc_retrieve_list_grouped",
        "pc_retrieve_topk_grouped_bf16", "pc_retrieve_list_grouped_bf16", "pc_retrieve_topk_grouped_biased")
RANK = ("pc_rank_grouped", "pc_rank_grouped_biased", "pc_rank_grouped_bf16", "pc_rank_grouped_where", "pc_rank_grouped_bf16_where")

# the entries' arguments in the order of the C ABI (include/pcompanion_hip.h)
ARGS = {
    "pc_retrieve_topk_grouped": "proj types rows type_rowptr type_col table n_types n dim slices out_idx out_score ws ws_bytes stream",
    "pc_retrieve_topk_grouped_excluding": "proj types row_key rows type_rowptr type_col table n_types ex_rowptr ex_col n_keys n dim "
                                          "slices out_idx out_score bad_count ws ws_bytes stream",
    "pc_retrieve_list_grouped": "proj types row_key rows type_rowptr type_col table n_types ex_rowptr ex_col n_keys n dim slices "
                                "out_idx out_score bad_count ws ws_bytes stream",
    "pc_retrieve_topk_grouped_bf16": "proj types row_key rows type_rowptr type_col table n_types ex_rowptr ex_col n_keys n dim slices "
                                     "out_idx out_score bad_count ws ws_bytes stream",
    "pc_retrieve_list_grouped_bf16": "proj types row_key rows type_rowptr type_col table n_types ex_rowptr ex_col n_keys n dim slices "
                                     "out_idx out_score bad_count ws ws_bytes stream",
    "pc_retrieve_topk_grouped_biased": "proj types row_key rows type_rowptr type_col table bias n_types ex_rowptr ex_col n_keys n dim "
                                       "slices out_idx out_score bad_count ws ws_bytes stream",
    "pc_rank_grouped": "proj types targets rows type_rowptr type_col table n_types num_products dim slices rank_out bad_count ws "
                       "ws_bytes stream",
    "pc_rank_grouped_excluding": "proj types targets row_key rows type_rowptr type_col table n_types num_products ex_rowptr ex_col "
                                 "n_keys cand_type dim slices rank_out bad_count ws ws_bytes stream",
    "pc_rank_grouped_biased": "proj types targets row_key rows type_rowptr type_col table bias n_types num_products ex_rowptr ex_col "
                              "n_keys cand_type dim slices rank_out bad_count ws ws_bytes stream",
    "pc_rank_grouped_bf16": "proj types targets row_key rows type_rowptr type_col table bias n_types num_products ex_rowptr ex_col "
                            "n_keys cand_type dim slices rank_out bad_count ws ws_bytes stream",
    "pc_rank_grouped_where": "proj types targets row_key rows type_rowptr type_col table bias n_types num_products ex_rowptr ex_col "
                             "n_keys cand_type dim slices rank_out bad_count where ws ws_bytes stream",
    "pc_rank_grouped_bf16_where": "proj types targets row_key rows type_rowptr type_col table bias n_types num_products ex_rowptr "
                                  "ex_col n_keys cand_type dim slices rank_out bad_count where ws ws_bytes stream",
}
INTS = {"rows": (4, 0, -1), "n_types": (3, 0, -1), "num_products": (9, 0, -1), "n_keys": (2, 0, -1), "n": (10, 0, 1, 16, 17, 256, 257),
        "dim": (128, 256, 64, 192, 0), "slices": (0, 1, 64, -1, 65)}
LISTS = ("row_key", "ex_rowptr", "ex_col", "bad_count", "cand_type")


def bind(path):
    L = ctypes.CDLL(path)
    for name in list(ARGS) + [e + "_workspace_bytes" for e in TOPN + RANK]:
        f = getattr(L, name)
        f.restype, f.argtypes = _lib.SIGNATURES[name]
    return L


def sizes(L):
    out = {}
    for r, t, s in itertools.product(ROWS, TYPES, SLICES):
        for e in RANK:
            out[e, r, t, s] = getattr(L, e + "_workspace_bytes")(r, t, s)
        for e, n in itertools.product(TOPN, NS):
            out[e, r, t, n, s] = getattr(L, e + "_workspace_bytes")(r, t, n, s)
    return out


def cases(entry, base):
    """argument dicts that the entry must refuse: `base` is valid but for a workspace of 0 bytes"""
    names = ARGS[entry].split()
    ptrs = [a for a in names if a not in INTS and a not in ("ws_bytes", "stream")]
    ints = [a for a in names if a in INTS]
    lists = [a for a in names if a in LISTS]
    yield {}
    for a in ptrs:
        yield {a: None}
    for a in ints:
        for v in INTS[a][1:]:
            yield {a: v}
    for a, b in itertools.combinations(ptrs + ints, 2):               # two changes at once: which check comes first
        for va in ((None,) if a in ptrs else INTS[a][1:]):
            for vb in ((None,) if b in ptrs else INTS[b][1:]):
                yield {a: va, b: vb}
    for absent in itertools.product((False, True), repeat=len(lists)):  # the exclusion arguments, all or none
        for nk in INTS["n_keys"] if "n_keys" in names else (None,):
            kw = {a: None for a, gone in zip(lists, absent) if gone}
            if nk is not None:
                kw["n_keys"] = nk
            for more in ({}, {"rows": 0}, {"n": 0}, {"dim": 192}):
                yield {**kw, **{k: v for k, v in more.items() if k in names}}
    if "bf16" in entry:                                               # a table that is not 16-byte aligned
        for off in (2, 8):
            for more in ({}, {"n": 17}, {"dim": 192}, {"slices": 65}, {"rows": 0}, {"bias": None},
                         {"row_key": None, "ex_rowptr": None, "ex_col": None, "n_keys": 0},
                         {"row_key": None, "ex_rowptr": None, "ex_col": None, "cand_type": None, "n_keys": 0}):
                yield {"table": ctypes.c_void_p(base["table"].value + off), **{k: v for k, v in more.items() if k in names}}
    if "where" in names:                                              # every present / absent shape of the pc_row_where
        fields = [f for f, _ in _lib.RowWhere._fields_]
        for present in itertools.product((False, True), repeat=len(fields)):
            where = _lib.RowWhere(**{f: base["table"].value for f, on in zip(fields, present) if on})
            for more in ({}, {"rows": 0}, {"dim": 192}, {"row_key": None}):
                yield {"where": ctypes.pointer(where), **more}


def run(L, entry, base, kw):
    a = {**base, **kw}
    n = a.get("n", 0)
    if a["ws_bytes"] is None:                                          # one byte short of what the entry asks for
        q = getattr(L, (entry if entry in TOPN + RANK else "pc_rank_grouped") + "_workspace_bytes")
        need = q(a["rows"], a["n_types"], n, a["slices"]) if entry in TOPN else q(a["rows"], a["n_types"], a["slices"])
        a["ws_bytes"] = max(need - 1, 0)
    return getattr(L, entry)(*a.values())


def main(parent, child):
    P, C = bind(parent), bind(child)
    sp, sc = sizes(P), sizes(C)
    differ = [k for k in sp if sp[k] != sc[k]]
    print(f"workspace queries: {len(sp)} calls of {len(TOPN) + len(RANK)} queries (rows {ROWS}, n_types {TYPES}, n {NS}, "
          f"slices {SLICES}), {sum(v == 0 for v in sp.values())} refused with 0, {len(differ)} differ")
    for k in differ[:20]:
        print("  DIFFERS", k, sp[k], sc[k])
    print(f"checksum of the parent's values: {sum(sp.values())}")
    bad = len(differ)
    buf = ctypes.create_string_buffer(96)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)              # passes every check; no check dereferences it
    print("refused calls (entry | calls | parent's codes | differ from the parent | not refused by the parent)")
    for entry, names in ARGS.items():
        hist, diff, launched, count = collections.Counter(), 0, 0, 0
        for short in (0, None):                                        # a workspace of 0 bytes; one byte short
            base = {a: (INTS[a][0] if a in INTS else p) for a in names.split()}
            if "where" in base:
                base["where"] = ctypes.pointer(_lib.RowWhere())         # every part absent: every product passes
            base.update(ws_bytes=short, stream=None)
            for kw in cases(entry, base):
                a, b = run(P, entry, base, kw), run(C, entry, base, kw)
                count += 1
                hist[a] += 1
                diff += a != b
                launched += a >= 0
                if a != b or a >= 0:
                    print("  MISMATCH" if a != b else "  NOT REFUSED", entry, kw, a, b)
        bad += diff + launched
        print(f"{entry} | {count} | {dict(sorted(hist.items(), reverse=True))} | {diff} | {launched}")
    print("verdict:", "equal" if not bad else f"{bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
