#!/usr/bin/env python3
"""Two builds of libpcompanion_hip.so side by side, no device involved: every pc_p2v_*_workspace_bytes* value over a grid of
shapes, and the return code of every refused call of tests/test_block_launchers_host.py's list.

    python scripts/dev/block_launchers_side_by_side.py PARENT.so CHILD.so > profiles/refactor_blocks_host.txt

Exit status 1 when anything differs, or when a listed call is not refused by the parent (it would launch)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_block_launchers_host as T                                   # noqa: E402
from p_companion_amd import _lib                                        # noqa: E402

EDGES = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
N_KEYS = (0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 467, 468)


def sizes(L):
    for name in ("pc_p2v_ffn_workspace_bytes", "pc_p2v_attention_workspace_bytes", "pc_p2v_attention_workspace_bytes_dim",
                 "pc_p2v_train_step_workspace_bytes", "pc_p2v_train_step_workspace_bytes_dim", "pc_p2v_export_workspace_bytes"):
        f = getattr(L, name)
        f.restype, f.argtypes = _lib.SIGNATURES[name]
    out = {}
    for r in EDGES + (0, -1, 8191, 8192, 86401, 1 << 20):
        out["ffn", r] = L.pc_p2v_ffn_workspace_bytes(r)
        for d in (64, 128, 256):
            out["export", r, d] = L.pc_p2v_export_workspace_bytes(r, d)
    for b in EDGES:
        for n in N_KEYS:
            out["attn", b, n] = L.pc_p2v_attention_workspace_bytes(b, n)
            for d in (128, 256):
                out["attn_dim", b, n, d] = L.pc_p2v_attention_workspace_bytes_dim(b, n, d)
            for k in range(1, 9):
                out["step", b, n, k] = L.pc_p2v_train_step_workspace_bytes(b, n, k)
                for d in (128, 256):
                    out["step_dim", b, n, k, d] = L.pc_p2v_train_step_workspace_bytes_dim(b, n, k, d)
    return out


def main(parent, child):
    P, C = T.bind(parent), T.bind(child)
    sp, sc = sizes(P), sizes(C)
    differ = [k for k in sp if sp[k] != sc[k]]
    print(f"workspace queries: {len(sp)} shapes (batch / rows {EDGES[0]}..{EDGES[-1]}, n {N_KEYS[0]}..{N_KEYS[-1]}, k 1..8, dim 128 / 256), "
          f"{len(differ)} differ")
    for k in differ[:20]:
        print("  DIFFERS", k, sp[k], sc[k])
    print(f"checksum of the parent's values: {sum(sp.values())}")
    print()
    print(f"refused calls: {len(T.CASES)}   (entry | what is wrong | parent | child | pinned in the test)")
    bad = len(differ)
    for entry, what, over, pinned in T.CASES:
        a, b = T.run_case(P, entry, over), T.run_case(C, entry, over)
        flag = "" if a == b == pinned and a < 0 else "   <-- MISMATCH"
        bad += bool(flag)
        print(f"{entry} | {what} | {a} | {b} | {pinned}{flag}")
    print()
    print("verdict:", "equal" if not bad else f"{bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
