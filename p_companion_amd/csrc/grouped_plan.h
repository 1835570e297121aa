// What the type-grouped catalogue kernels share (retrieve*.hip, nearest.hip: the top n of a type; rank.hip, nearest.hip: the
// rank of one product in it): the chunk and slice constants, the slice plan, the total order of (score, product), and on the
// host the entries' checks, their workspace, the planning launches that gather the rows of a type into tiles (grouped_plan.hip)
// and the merge of the slices' partial lists (retrieve.hip).  The device helpers of the score kernels: grouped_select.h.
#pragma once
#include "common.h"

#define RG_NONE 0x7fffffff
#define RG_AUTO_SLICES 16
#define RG_MAX_SLICES 64
#define RG_SLICE_MIN 4096          // candidates a slice gets at least (fewer slices for a small type)
#define RG_CHUNK 64                // candidates per chunk: four waves x 16
#define RG_MAX_GRID 4096

// Slices of a type with C candidates at most S slices: ns slices of L candidates (L a multiple of the chunk, the last slice
// shorter), none empty.  Host and device use the same arithmetic.
__host__ __device__ __forceinline__ void rg_slice_plan(int C, int S, int& ns, int& L) {
    if (C <= 0) { ns = 0; L = 0; return; }
    int want = (C + RG_SLICE_MIN - 1) / RG_SLICE_MIN;
    if (want > S) want = S;
    const int per = (C + want - 1) / want;
    L = (per + RG_CHUNK - 1) / RG_CHUNK * RG_CHUNK;
    ns = (C + L - 1) / L;
}

// (score descending, product index ascending)
__device__ __forceinline__ bool rg_better(float x, int xi, float y, int yi) { return x > y || (x == y && xi < yi); }

// ---- the plan: rows grouped by type, work items (type, slice, tile) -------------------------------------------------
// The five planning arrays at the head of every workspace: cnt [n_types], pos [rows], row_start [n_types + 1],
// item_start [n_types + 1], order [rows].
struct RgPlan {
    int32_t *cnt, *pos, *row_start, *order;
    int64_t* item_start;
};
RgPlan rg_plan_carve(WsCarver& cv, int rows, int n_types);
// slices as the entry points take it (0: the default) -> S
inline int rg_slices(int slices) { return slices == 0 ? RG_AUTO_SLICES : slices; }
// memset, count, scan, place on `st` (tiles of TM rows, at most S slices); the launches' status is left to the caller's
// pc_launch_status().  pos[r] = -1 for a row that takes no part: types[r] outside [0, n_types), or -- with targets --
// targets[r] outside [0, num_products); a row with a type and an id out of range is counted in *bad_count.  targets,
// rank_out (set to 0, or -1 beside pos) and bad_count may be null.
int rg_plan_launch(const RgPlan& w, const int32_t* types, const int32_t* targets, int rows, const int32_t* type_rowptr,
                   int n_types, int num_products, int S, int TM, int32_t* rank_out, int32_t* bad_count, hipStream_t st);
// the hot kernel's grid: at most (tiles over all rows + one partial tile per type) x S items; the kernel reads the real count
unsigned rg_item_grid(int rows, int n_types, int S, int TM);

// ---- what the entries share on the host ------------------------------------------------------------------------------
// An entry's workspace: the plan, then the slices' partial lists pv / pi [rows][S][n] at the rows' grouped positions (n = 0, the
// rank entries: the plan alone).
struct RgWs {
    RgPlan plan;
    float* pv;
    int32_t* pi;
    size_t bytes;
};
RgWs rg_ws_carve(void* ws, int rows, int n_types, int n, int S);
// a top-n entry's workspace query (lists of up to max_n): 0 for a shape the entry refuses
size_t rg_topn_workspace_bytes(int rows, int n_types, int n, int max_n, int slices);
// An entry's optional exclusion lists come all or none (bad_count is needed with them and may be given without).
inline bool rg_lists_ok(const int32_t* row_key, const int32_t* ex_rowptr, const int32_t* ex_col, const int32_t* bad_count, int n_keys) {
    return row_key ? ex_rowptr && ex_col && bad_count && n_keys >= 0 : !ex_rowptr && !ex_col && n_keys == 0;
}
// The top-n entries' checks in their order: the entry's own null checks (args_ok), the counts and its lists (PC_EINVAL), then
// the shapes (PC_ESHAPE).
inline int rg_topn_check(bool args_ok, int rows, int n_types, bool lists_ok, int n, int max_n, int dim, int slices) {
    if (!args_ok || rows <= 0 || n_types <= 0 || !lists_ok) return PC_EINVAL;
    if (n < 1 || n > max_n || (dim != 128 && dim != 256) || slices < 0 || slices > RG_MAX_SLICES) return PC_ESHAPE;
    return PC_OK;
}
// Between an entry's checks and its hot kernel: the workspace carved into w and checked against ws_bytes (PC_EWORKSPACE), the
// plan launched (rg_plan_launch's arguments), the hot kernel's grid.
int rg_begin(RgWs& w, unsigned& grid, void* ws, size_t ws_bytes, const int32_t* types, const int32_t* targets, int rows,
             const int32_t* type_rowptr, int n_types, int num_products, int n, int S, int TM, int32_t* rank_out,
             int32_t* bad_count, hipStream_t st);
// rg_merge_kernel (retrieve.hip), one wave per row: the top n <= RG_MAX_N of the row's slices' partial lists -> out_idx / out_score [rows][n]
// (-1 / -inf past the end of a short list).
void rg_merge_launch(const RgWs& w, const int32_t* types, int rows, const int32_t* type_rowptr, int n_types, int n, int S,
                     int32_t* out_idx, float* out_score, hipStream_t st);
