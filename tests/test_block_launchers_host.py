"""The argument checks of the FFN and attention block launchers, without a GPU: every stand-alone entry is called with
pointers that are never dereferenced on the way to a refusal, and the return code of each refused call is pinned -- one call
per check of each launcher, and calls that break two checks at once, which fixes the ORDER of the checks (the order decides
which code a doubly wrong call returns, so it is behaviour).  The expected codes were taken from the library of the commit
BEFORE the launchers took call blocks (profiles/refactor_blocks_host.txt, written by scripts/dev/block_launchers_side_by_side.py,
which runs this same list against two libraries); no call in the list gets as far as a launch."""
import ctypes

import pytest

PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE, PC_EBATCHNORM = -1, -2, -3, -4
X = 4096                                            # stands for a device pointer
N_LDS = 469                                         # 8 * HEADS * N floats of scores + dropout multipliers pass 60000 bytes of LDS

# argument order of each entry (include/pcompanion_hip.h)
ORDER = {
    "pc_p2v_ffn_forward_train": "p table idx rows seg update_running y ffn_sv ws ws_bytes stream",
    "pc_p2v_ffn_forward_eval": "p table idx rows y ws ws_bytes stream",
    "pc_p2v_ffn_backward": "p g table idx rows seg dy ffn_sv dx accumulate ws ws_bytes stream",
    "pc_p2v_attention_forward": "p query keys B N out attn_sv ws ws_bytes stream",
    "pc_p2v_attention_backward": "p g query keys B N dout attn_sv dquery dkeys accumulate ws ws_bytes stream",
    "pc_p2v_attention_forward_masked": "p query keys key_pad B N out attn_sv ws ws_bytes stream",
    "pc_p2v_attention_backward_masked": "p g query keys key_pad B N dout attn_sv dquery dkeys accumulate ws ws_bytes stream",
    "pc_p2v_train_step_compact_masked": "p g table anchor positive negative nb_rows n_real slot_row B N K margin loss d_pos d_neg "
                                        "anchor_emb profile ws ws_bytes stream",
    "pc_p2v_train_step_unique_masked": "p g table anchor positive negative step_rows nb_rows nb_weight n_unique n_real_slots slot_row "
                                       "ref_off ref_slot B N K margin loss d_pos d_neg anchor_emb profile ws ws_bytes adam stream",
}
FFN_TRAIN, FFN_EVAL, FFN_BWD, ATT_FWD, ATT_BWD, ATT_FWD_M, ATT_BWD_M, STEP_CM, STEP_UM = ORDER

# (entry, what is wrong, overrides of a call that would otherwise pass every check, the refusal's code).  Overrides: an argument
# by name (None = NULL); dim = PRODUCT_EMB_DIM in the parameter struct; p_null / g_null / sv_null = fields left NULL;
# seg_bad = segments that do not end at `rows`; ws_bytes "short" / "exact" = one byte less than / exactly what the entry's
# workspace query answers.
CASES = [
    # ---- ffn forward (train): !y, then ffn_check (pointers and rows, dim, weights, segments, workspace), then the saved block
    (FFN_TRAIN, "no y", dict(y=None), PC_EINVAL),
    (FFN_TRAIN, "no p", dict(p=None), PC_EINVAL),
    (FFN_TRAIN, "no table", dict(table=None), PC_EINVAL),
    (FFN_TRAIN, "rows = 0", dict(rows=0), PC_EINVAL),
    (FFN_TRAIN, "no ws", dict(ws=None), PC_EINVAL),
    (FFN_TRAIN, "dim = 64", dict(dim=64), PC_ESHAPE),
    (FFN_TRAIN, "no w3", dict(p_null=("w3",)), PC_EINVAL),
    (FFN_TRAIN, "segments end elsewhere", dict(seg_bad=True), PC_EINVAL),
    (FFN_TRAIN, "workspace one byte short", dict(ws_bytes="short"), PC_EWORKSPACE),
    (FFN_TRAIN, "no saved block", dict(ffn_sv=None), PC_EINVAL),
    (FFN_TRAIN, "no saved h0", dict(sv_null=("h0",)), PC_EINVAL),
    (FFN_TRAIN, "exact workspace, no saved bn_shift", dict(ws_bytes="exact", sv_null=("bn_shift",)), PC_EINVAL),
    (FFN_TRAIN, "no y + dim = 64", dict(y=None, dim=64), PC_EINVAL),
    (FFN_TRAIN, "no table + dim = 64", dict(table=None, dim=64), PC_EINVAL),
    (FFN_TRAIN, "dim = 64 + no weights", dict(dim=64, p_null=("w0", "b0", "w3", "b3", "w5", "b5", "gamma", "beta")), PC_ESHAPE),
    (FFN_TRAIN, "dim = 64 + short workspace", dict(dim=64, ws_bytes="short"), PC_ESHAPE),
    (FFN_TRAIN, "bad segments + short workspace", dict(seg_bad=True, ws_bytes="short"), PC_EINVAL),
    (FFN_TRAIN, "short workspace + no saved block", dict(ws_bytes="short", ffn_sv=None), PC_EWORKSPACE),
    (FFN_TRAIN, "dim = 256, short workspace", dict(dim=256, ws_bytes="short"), PC_EWORKSPACE),
    # ---- ffn forward (eval): ffn_check without segments, then y and the running statistics
    (FFN_EVAL, "no p", dict(p=None), PC_EINVAL),
    (FFN_EVAL, "rows = -1", dict(rows=-1), PC_EINVAL),
    (FFN_EVAL, "dim = 64", dict(dim=64), PC_ESHAPE),
    (FFN_EVAL, "no b5", dict(p_null=("b5",)), PC_EINVAL),
    (FFN_EVAL, "workspace one byte short", dict(ws_bytes="short"), PC_EWORKSPACE),
    (FFN_EVAL, "no y", dict(y=None), PC_EINVAL),
    (FFN_EVAL, "no running_var", dict(p_null=("running_var",)), PC_EINVAL),
    (FFN_EVAL, "dim = 64 + no y", dict(dim=64, y=None), PC_ESHAPE),
    (FFN_EVAL, "short workspace + no y", dict(ws_bytes="short", y=None), PC_EWORKSPACE),
    (FFN_EVAL, "short workspace + no running_mean", dict(ws_bytes="short", p_null=("running_mean",)), PC_EWORKSPACE),
    # ---- ffn backward: ffn_check, then g / dy / the saved block, then g's fields
    (FFN_BWD, "no p", dict(p=None), PC_EINVAL),
    (FFN_BWD, "no table", dict(table=None), PC_EINVAL),
    (FFN_BWD, "dim = 64", dict(dim=64), PC_ESHAPE),
    (FFN_BWD, "no gamma", dict(p_null=("gamma",)), PC_EINVAL),
    (FFN_BWD, "segments end elsewhere", dict(seg_bad=True), PC_EINVAL),
    (FFN_BWD, "workspace one byte short", dict(ws_bytes="short"), PC_EWORKSPACE),
    (FFN_BWD, "no g", dict(g=None), PC_EINVAL),
    (FFN_BWD, "no dy", dict(dy=None), PC_EINVAL),
    (FFN_BWD, "no saved block", dict(ffn_sv=None), PC_EINVAL),
    (FFN_BWD, "no saved a2", dict(sv_null=("a2",)), PC_EINVAL),
    (FFN_BWD, "no g.w5", dict(g_null=("w5",)), PC_EINVAL),
    (FFN_BWD, "dim = 64 + no dy", dict(dim=64, dy=None), PC_ESHAPE),
    (FFN_BWD, "short workspace + no g", dict(ws_bytes="short", g=None), PC_EWORKSPACE),
    (FFN_BWD, "short workspace + no g.b0, accumulate", dict(ws_bytes="short", g_null=("b0",), accumulate=1), PC_EWORKSPACE),
    (FFN_BWD, "rows = 0 + dim = 64", dict(rows=0, dim=64), PC_EINVAL),
    # ---- attention forward: attn_check (key rows, parameters, dim, sizes and the saved block, LDS, workspace), then query / keys / out
    (ATT_FWD, "B = 0", dict(B=0), PC_EINVAL),
    (ATT_FWD, "N = 0", dict(N=0), PC_EINVAL),
    (ATT_FWD, "no p", dict(p=None), PC_EINVAL),
    (ATT_FWD, "no out_proj_b", dict(p_null=("out_proj_b",)), PC_EINVAL),
    (ATT_FWD, "dim = 64", dict(dim=64), PC_ESHAPE),
    (ATT_FWD, "B, N < 0", dict(B=-2, N=-3), PC_EINVAL),
    (ATT_FWD, "no saved block", dict(attn_sv=None), PC_EINVAL),
    (ATT_FWD, "no saved probs", dict(sv_null=("probs",)), PC_EINVAL),
    (ATT_FWD, "no ws", dict(ws=None), PC_EINVAL),
    (ATT_FWD, "scores exceed LDS", dict(N=N_LDS), PC_ESHAPE),
    (ATT_FWD, "the largest N, short workspace", dict(N=N_LDS - 1, ws_bytes="short"), PC_EWORKSPACE),
    (ATT_FWD, "workspace one byte short", dict(ws_bytes="short"), PC_EWORKSPACE),
    (ATT_FWD, "dim = 256, short workspace", dict(dim=256, ws_bytes="short"), PC_EWORKSPACE),
    (ATT_FWD, "no query", dict(query=None), PC_EINVAL),
    (ATT_FWD, "no keys", dict(keys=None), PC_EINVAL),
    (ATT_FWD, "exact workspace, no out", dict(ws_bytes="exact", out=None), PC_EINVAL),
    (ATT_FWD, "dim = 64 + no in_proj_w", dict(dim=64, p_null=("in_proj_w",)), PC_EINVAL),
    (ATT_FWD, "dim = 64 + no saved block", dict(dim=64, attn_sv=None), PC_ESHAPE),
    (ATT_FWD, "dim = 64 + B, N < 0", dict(dim=64, B=-2, N=-3), PC_ESHAPE),
    (ATT_FWD, "no saved block + scores exceed LDS", dict(attn_sv=None, N=N_LDS), PC_EINVAL),
    (ATT_FWD, "scores exceed LDS + short workspace", dict(N=N_LDS, ws_bytes=0), PC_ESHAPE),
    (ATT_FWD, "short workspace + no query", dict(ws_bytes="short", query=None), PC_EWORKSPACE),
    # ---- attention backward: attn_check, then g and its fields, then the five pointers
    (ATT_BWD, "N = 0", dict(N=0), PC_EINVAL),
    (ATT_BWD, "no p", dict(p=None), PC_EINVAL),
    (ATT_BWD, "dim = 64", dict(dim=64), PC_ESHAPE),
    (ATT_BWD, "no saved ctx", dict(sv_null=("ctx",)), PC_EINVAL),
    (ATT_BWD, "scores exceed LDS", dict(N=N_LDS), PC_ESHAPE),
    (ATT_BWD, "workspace one byte short", dict(ws_bytes="short"), PC_EWORKSPACE),
    (ATT_BWD, "no g", dict(g=None), PC_EINVAL),
    (ATT_BWD, "no g.in_proj_b", dict(g_null=("in_proj_b",)), PC_EINVAL),
    (ATT_BWD, "no dout", dict(dout=None), PC_EINVAL),
    (ATT_BWD, "no dquery", dict(dquery=None), PC_EINVAL),
    (ATT_BWD, "exact workspace, no dkeys, accumulate", dict(ws_bytes="exact", dkeys=None, accumulate=1), PC_EINVAL),
    (ATT_BWD, "dim = 64 + no g", dict(dim=64, g=None), PC_ESHAPE),
    (ATT_BWD, "short workspace + no g", dict(ws_bytes="short", g=None), PC_EWORKSPACE),
    (ATT_BWD, "scores exceed LDS + no keys", dict(N=N_LDS, keys=None), PC_ESHAPE),
    # ---- the masked attention entries: key_pad, B, N in the entry itself, then as above
    (ATT_FWD_M, "no key_pad + dim = 64", dict(key_pad=None, dim=64), PC_EINVAL),
    (ATT_FWD_M, "dim = 64", dict(dim=64), PC_ESHAPE),
    (ATT_FWD_M, "scores exceed LDS", dict(N=N_LDS), PC_ESHAPE),
    (ATT_FWD_M, "workspace one byte short", dict(ws_bytes="short"), PC_EWORKSPACE),
    (ATT_FWD_M, "short workspace + no out", dict(ws_bytes="short", out=None), PC_EWORKSPACE),
    (ATT_FWD_M, "no out", dict(out=None), PC_EINVAL),
    (ATT_BWD_M, "no key_pad + short workspace", dict(key_pad=None, ws_bytes="short"), PC_EINVAL),
    (ATT_BWD_M, "dim = 64", dict(dim=64), PC_ESHAPE),
    (ATT_BWD_M, "dim = 256, short workspace", dict(dim=256, ws_bytes="short"), PC_EWORKSPACE),
    (ATT_BWD_M, "no g", dict(g=None), PC_EINVAL),
    (ATT_BWD_M, "no dkeys", dict(dkeys=None), PC_EINVAL),
    # ---- the masked steps: the dim check and the workspace check sit behind the step's own argument checks
    (STEP_CM, "dim = 64", dict(dim=64), PC_ESHAPE),
    (STEP_CM, "workspace one byte short", dict(ws_bytes="short"), PC_EWORKSPACE),
    (STEP_CM, "dim = 256, short workspace", dict(dim=256, ws_bytes="short"), PC_EWORKSPACE),
    (STEP_CM, "one real slot + dim = 64", dict(n_real=1, dim=64), PC_EBATCHNORM),
    (STEP_CM, "no loss + dim = 64", dict(loss=None, dim=64), PC_EINVAL),
    (STEP_CM, "dim = 64 + short workspace", dict(dim=64, ws_bytes=0), PC_ESHAPE),
    (STEP_UM, "dim = 64", dict(dim=64), PC_ESHAPE),
    (STEP_UM, "workspace one byte short", dict(ws_bytes="short"), PC_EWORKSPACE),
    (STEP_UM, "B = 1 + dim = 64", dict(B=1, n_unique=1, n_real_slots=2, dim=64), PC_EBATCHNORM),
]


def bind(path):
    """The entries of the library at `path`, with the argument types the package binds them with."""
    from p_companion_amd import _lib
    L = ctypes.CDLL(path)
    names = list(ORDER) + ["pc_p2v_ffn_workspace_bytes", "pc_p2v_attention_workspace_bytes_dim", "pc_p2v_train_step_workspace_bytes_dim"]
    for name in names:
        f = getattr(L, name)
        f.restype, f.argtypes = _lib.SIGNATURES[name]
    return L


def _filled(cls, null=(), dim=None):
    s = cls()
    for name, ctype in cls._fields_:
        if ctype is ctypes.c_void_p and name not in null:
            setattr(s, name, X)
    if dim is not None:
        s.dim = dim
    return s


def run_case(L, entry, over):
    """The return code of `entry` for a call that passes every check except what `over` breaks."""
    from p_companion_amd import _lib
    over = dict(over)
    dim = over.pop("dim", 0)
    ffn = "ffn" in entry
    sv_null = over.pop("sv_null", ())
    p = _filled(_lib.P2VTensors, over.pop("p_null", ()), dim)
    g = _filled(_lib.P2VTensors, over.pop("g_null", ()), dim)
    ffn_sv, attn_sv = _filled(_lib.FfnSaved, sv_null if ffn else ()), _filled(_lib.AttnSaved, () if ffn else sv_null)
    v = dict(p=ctypes.byref(p), g=ctypes.byref(g), ffn_sv=ctypes.byref(ffn_sv), attn_sv=ctypes.byref(attn_sv), rows=200,
             update_running=0, accumulate=0, B=4, N=3, K=5, margin=1.0, n_real=6, n_unique=5, n_real_slots=9, ws_bytes=1 << 40,
             stream=None, profile=None, adam=None, step_rows=None)
    if entry.startswith("pc_p2v_train_step"):
        v.update(B=8, N=4)
    v.update(over)
    seg = _lib.Segments()
    seg.nseg, seg.weighted_row, seg.weight = 2, -1, 1.0
    seg.start[0], seg.start[1], seg.start[2] = 0, 120, v["rows"] + (1 if v.pop("seg_bad", False) else 0)
    v["seg"] = ctypes.byref(seg)
    if v["ws_bytes"] in ("short", "exact"):
        d = 256 if dim == 256 else 128
        need = (L.pc_p2v_ffn_workspace_bytes(v["rows"]) if ffn else
                L.pc_p2v_train_step_workspace_bytes_dim(v["B"], v["N"], v["K"], d) if entry.startswith("pc_p2v_train_step") else
                L.pc_p2v_attention_workspace_bytes_dim(v["B"], v["N"], d))
        assert need > 0, (entry, over)
        v["ws_bytes"] = need - (1 if v["ws_bytes"] == "short" else 0)
    return getattr(L, entry)(*[v.get(name, X) for name in ORDER[entry].split()])


@pytest.fixture(scope="module")
def library():
    from p_companion_amd import _lib
    return bind(_lib.LIB_PATH)


@pytest.mark.parametrize("entry", list(ORDER))
def test_refused_calls_return_the_pinned_codes(library, entry):
    cases = [c for c in CASES if c[0] == entry]
    assert cases
    got = [(what, run_case(library, entry, over)) for _, what, over, _ in cases]
    assert got == [(what, code) for _, what, _, code in cases]


def test_every_pinned_code_is_a_refusal():
    # a call that passed the checks would launch on pointers that stand for nothing
    assert all(code in (PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE, PC_EBATCHNORM) for *_, code in CASES)
    assert {PC_EWORKSPACE, PC_ESHAPE} <= {code for *_, code in CASES}
