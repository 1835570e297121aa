// What the long-list entries share (retrieve_list.hip: the fp32 table; retrieve_list_bf16.hip: the bf16 copy): the list and
// buffer sizes of the per-row selection, and on the host the merge of the slices' sorted partial lists (retrieve_list.hip).
#pragma once
#include "grouped_plan.h"

#define RL_MAX_N 256
#define RL_N2 32                   // n up to here: 128 buffer entries per row (NE = 2); a compacted row has 32 entries of slack
#define RL_N4 96                   // n up to here: 256 entries (NE = 4), 96 of slack; above: RL_CAP (NE = 8), 128 at n = 256
#define RL_TM 16                   // rows per tile
#define RL_CAP 448                 // buffer entries per row of the long variant: n + three chunks at n = 256

// rl_merge_kernel (retrieve_list.hip), one wave per row: the first n <= RL_MAX_N of the row's slices' sorted partial lists
// w.pv / w.pi [rows][S][n] -> out_idx / out_score [rows][n] (-1 / -inf past the end of a short list).
void rl_merge_launch(const RgWs& w, const int32_t* types, int rows, const int32_t* type_rowptr, int n_types, int n, int S,
                     int32_t* out_idx, float* out_score, hipStream_t st);
