#!/usr/bin/env python3
"""Two trees' Python serving layer side by side, no device and no library involved: the public names of ops.py and
inference.py, the inspect.signature of every public function and method in them, and the interpreter work (Python calls, C calls
and bytecodes of one call, counted with sys.setprofile and opcode tracing: deterministic) and the host time per call of the grouped
wrappers with the stand-ins of tests/test_grouped_wrappers_host.py (host tensors that report is_cuda, a library whose entries
return at once, one fixed workspace and stream) -- so what is timed is the wrappers' own Python, nothing else.

    python scripts/dev/grouped_wrappers_side_by_side.py PARENT_TREE [CHILD_TREE] [--calls 4000] [--rounds 8] [--out FILE]

Six cases (plain retrieval, biased + exclude retrieval, list + exclude, and biased + exclude rank over the fp32 table, over the
bf16 copy and under a full predicate) at R = 6 rows, P = 9 products, D = 128; `--rounds` rounds, the two trees alternating inside a round, calls / rounds calls of a case at a time.  The subclass
inflates the absolute times and the rounds of one process vary by tens of per cent, so the times say little beside the counts;
only parent against child means anything.  Prints ONE JSON line and, with --out, writes it.
Exit status 1 when the public names or a signature differ."""
import argparse
import ctypes
import importlib.util
import inspect
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
R, P, T, D, KEYS = 6, 9, 3, 128, 4


def load(tree, alias):
    """The tree's p_companion_amd under the name `alias`, with ops and inference imported."""
    init = os.path.join(tree, "p_companion_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(alias, init, submodule_search_locations=[os.path.dirname(init)])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules[alias] = pkg
    spec.loader.exec_module(pkg)
    return importlib.import_module(alias + ".ops"), importlib.import_module(alias + ".inference")


def surface(module):
    """{public name: its signature, and for a class its public methods' -- or the value's type}"""
    out = {}
    sig = lambda f: str(inspect.signature(f)).replace(module.__name__.split(".")[0] + ".", "p_companion_amd.")   # (the alias)
    for name in sorted(n for n in dir(module) if not n.startswith("_")):
        obj = getattr(module, name)
        if inspect.isclass(obj) and obj.__module__ == module.__name__:
            out[name] = {m: sig(f) for m, f in inspect.getmembers(obj, callable)
                         if not m.startswith("_") and not inspect.isclass(f)}
        elif inspect.isfunction(obj):
            out[name] = sig(obj)
        else:
            out[name] = type(obj).__name__
    return out


class OnDevice(torch.Tensor):
    is_cuda = True


def dev(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)


class Library:
    def __getattr__(self, name):
        return lambda *args: 0


def cases(ops):
    library, stream, ws = Library(), ctypes.c_void_p(0x5EED0), dev(4096, dtype=torch.uint8)
    ops._lib.lib = lambda: library
    ops._stream = lambda: stream
    ops.workspace = lambda nbytes, device, tag="ws": ws
    i32 = torch.int32
    proj, types, targets = dev(R, D), dev(R, dtype=i32), dev(R, dtype=i32)
    rowptr, col, table, bias, cand = dev(T + 1, dtype=i32), dev(P, dtype=i32), dev(P, D), dev(P), dev(P, dtype=i32)
    exclude = (dev(R, dtype=i32), dev(KEYS + 1, dtype=i32), dev(5, dtype=i32))
    table16 = dev(P, D, dtype=torch.bfloat16)
    where = ops.RowWhere(value=dev(P), flags=dev(P, dtype=i32), lo=dev(R), hi=dev(R), need=dev(R, dtype=i32), deny=dev(R, dtype=i32))
    return {
        "retrieve_plain": lambda: ops.retrieve_topk_grouped(proj, types, rowptr, col, table, 10),
        "retrieve_biased_exclude": lambda: ops.retrieve_topk_grouped(proj, types, rowptr, col, table, 10, exclude=exclude, bias=bias),
        "list_exclude": lambda: ops.retrieve_list_grouped(proj, types, rowptr, col, table, 100, exclude=exclude),
        "rank_biased_exclude": lambda: ops.rank_grouped(proj, types, targets, rowptr, col, table, exclude=exclude, cand_type=cand,
                                                        bias=bias),
        "rank_bf16_biased_exclude": lambda: ops.rank_grouped_bf16(proj, types, targets, rowptr, col, table16, exclude=exclude,
                                                                  cand_type=cand, bias=bias),
        "rank_where_biased_exclude": lambda: ops.rank_grouped_where(proj, types, targets, rowptr, col, table, where, exclude=exclude,
                                                                    cand_type=cand, bias=bias),
    }


def work(fn):
    """[Python calls, C calls, bytecodes] of one fn()"""
    n = [0, 0, 0]

    def profile(frame, event, arg):
        n[0] += event == "call"
        n[1] += event == "c_call"

    def trace(frame, event, arg):
        frame.f_trace_opcodes = True
        n[2] += event == "opcode"
        return trace

    fn()
    sys.setprofile(profile)
    fn()
    sys.setprofile(None)
    sys.settrace(trace)
    fn()
    sys.settrace(None)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("child", nargs="?", default=ROOT)
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    trees = {"parent": load(args.parent, "pc_parent"), "child": load(args.child, "pc_child")}
    same = {}
    for i, module in enumerate(("ops", "inference")):
        a, b = surface(trees["parent"][i]), surface(trees["child"][i])
        same[module] = {"public_names": len(a), "names_equal": sorted(a) == sorted(b), "signatures_equal": a == b,
                        "differing": sorted(n for n in set(a) | set(b) if a.get(n) != b.get(n))}
    fns = {side: cases(mods[0]) for side, mods in trees.items()}
    per = max(args.calls // args.rounds, 1)
    host = {}
    for case in fns["parent"]:
        us = {"parent": [], "child": []}
        for side in us:
            fns[side][case]()
        for _ in range(args.rounds):
            for side in us:
                fn = fns[side][case]
                t0 = time.perf_counter()
                for _ in range(per):
                    fn()
                us[side].append((time.perf_counter() - t0) / per * 1e6)
        host[case] = {side: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                             "us_all": [round(x, 2) for x in v]} for side, v in us.items()}
        host[case]["child_over_parent"] = round(host[case]["child"]["median_us"] / host[case]["parent"]["median_us"], 4)
    counts = {case: {side: work(fns[side][case]) for side in fns} for case in fns["parent"]}
    res = {"probe": "grouped_wrappers_side_by_side", "calls_per_case": per * args.rounds, "rounds": args.rounds, "surface": same,
           "python_calls_c_calls_bytecodes_per_call": counts, "host_us_per_call": host}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if all(s["signatures_equal"] for s in same.values()) else 1)


if __name__ == "__main__":
    main()
