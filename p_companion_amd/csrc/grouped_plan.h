// What the type-grouped catalogue kernels share (retrieve.hip: the top n of a type; rank.hip: the rank of one product in it):
// the chunk and slice constants, the slice plan, the total order of (score, product) and the planning launches that gather
// the rows of a type into tiles (grouped_plan.hip).
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
// The five planning arrays at the head of both workspaces: cnt [n_types], pos [rows], row_start [n_types + 1],
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
