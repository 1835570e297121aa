// The rank of a known product among the products of its type that the row's exclusion list leaves (PCompanionInference with
// set_exclusions / set_eligible: rank_targets, evaluate_catalogue).  A unit of its own: in rank.hip the new kernel changed the
// register allocation of rk_rank_kernel<128>, and the unfiltered path keeps its text.
#include "common.h"
#include "grouped_plan.h"          // rg_better
#include "rank_chain.h"

// rk_rank_kernel runs as it is and counts over the whole type; this post-pass takes the excluded products out again.  One wave
// per row: the row's proj is row 0 of the A operand (rows 1..15 are zero: an MFMA's output row depends on its own A row alone),
// the B operand is blocks of 16 columns -- column 0 of the first block the target y, then the row's list ex_col[elo, ehi) --
// through rk_chain (the dimensions in index order), so g and every s_e are the bits rk_rank_kernel compared.  A list entry e
// with cand_type[e] == types[r] and rg_better(s_e, e, g, y) was counted there: one off.  e == y, or cand_type[y] != types[r]:
// the target is no candidate of the row, rank -1.  A row the plan left at -1 stays so; an id outside [0, num_products) is
// passed over; a key outside [-1, n_keys) is no list and is counted in *bad_count.  Integer work, the row's wave the one writer.
template <int D>
__global__ __launch_bounds__(64) void rk_exclude_kernel(const float* __restrict__ proj, const int32_t* __restrict__ types,
                                                        const int32_t* __restrict__ targets, const int32_t* __restrict__ row_key,
                                                        const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col,
                                                        int n_keys, const int32_t* __restrict__ cand_type,
                                                        const float* __restrict__ table, int num_products,
                                                        int32_t* __restrict__ rank_out, int32_t* __restrict__ bad_count) {
    constexpr int QS = RK_QS(D), NB = D / 16;
    __shared__ __attribute__((aligned(16))) float q[16 * QS];
    const int lane = threadIdx.x, c = lane & 15, h = lane >> 4;
    const int r = blockIdx.x;
    int key = row_key[r];
    if (key < -1 || key >= n_keys) {
        if (lane == 0) atomicAdd(bad_count, 1);
        key = -1;
    }
    const int base = rank_out[r];
    if (base < 0) return;                                 // (wave-uniform, as every exit below) no type, or an id out of range
    const int t = types[r], y = targets[r];               // both inside their ranges: the plan counted the row
    if (cand_type[y] != t) {
        if (lane == 0) rank_out[r] = -1;
        return;
    }
    if (key < 0) return;
    const int elo = ex_rowptr[key], len = ex_rowptr[key + 1] - elo;
    if (len <= 0) return;
    for (int e = lane; e < 16 * (QS / 4); e += 64) {
        const int row = e / (QS / 4), d4 = e - row * (QS / 4);
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row == 0 && d4 < D / 4) x = reinterpret_cast<const float4*>(proj + (size_t)r * D)[d4];
        *reinterpret_cast<float4*>(&q[row * QS + 4 * d4]) = x;
    }
    __syncthreads();
    float g = 0.f;
    int dec = 0;
    bool hit = false;
    for (int v0 = 0; v0 <= len; v0 += 16) {               // column v: the target (v == 0), list entry v - 1
        const int v = v0 + c;
        int id = -1;
        if (v == 0) id = y;
        else if (v <= len) id = ex_col[elo + v - 1];
        if (id >= num_products) id = -1;
        float4 b[NB];
        const float4* f = reinterpret_cast<const float4*>(table + (size_t)max(id, 0) * D) + h;
#pragma unroll
        for (int k = 0; k < NB; k++) b[k] = f[4 * k];
        f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
        rk_chain<D, 1>(q, 0, b, nullptr, acc, c, h);
        // C/D map of the 16x16 f32 MFMA: column lane & 15, row 4 (lane >> 4) + reg: row 0 is register 0 of lanes 0..15
        const float s = acc[0][0];
        if (v0 == 0) g = __shfl(s, 0, 64);
        const bool mine = h == 0 && v > 0 && id >= 0;
        hit |= __any(mine && id == y);
        dec += __popcll(__ballot(mine && id != y && cand_type[max(id, 0)] == t && rg_better(s, id, g, y)));
    }
    if (lane == 0) rank_out[r] = hit ? -1 : base - dec;
}

extern "C" int pc_rank_grouped_excluding(const float* proj, const int32_t* types, const int32_t* targets,
                                         const int32_t* row_key, int rows, const int32_t* type_rowptr,
                                         const int32_t* type_col, const float* table, int n_types, int num_products,
                                         const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, const int32_t* cand_type,
                                         int dim, int slices, int32_t* rank_out, int32_t* bad_count, void* ws, size_t ws_bytes,
                                         void* stream) {
    if (!row_key || !ex_rowptr || !ex_col || !cand_type || n_keys < 0) return PC_EINVAL;
    // every other check, the plan and rk_rank_kernel: the unfiltered entry as it is
    PC_TRY(pc_rank_grouped(proj, types, targets, rows, type_rowptr, type_col, table, n_types, num_products, dim, slices, rank_out,
                           bad_count, ws, ws_bytes, stream));
    hipStream_t st = (hipStream_t)stream;
    if (dim == 128)
        PC_LAUNCH(rk_exclude_kernel<128>, dim3(rows), dim3(64), 0, st, proj, types, targets, row_key, ex_rowptr, ex_col, n_keys,
                  cand_type, table, num_products, rank_out, bad_count);
    else
        PC_LAUNCH(rk_exclude_kernel<256>, dim3(rows), dim3(64), 0, st, proj, types, targets, row_key, ex_rowptr, ex_col, n_keys,
                  cand_type, table, num_products, rank_out, bad_count);
    return pc_launch_status();
}
