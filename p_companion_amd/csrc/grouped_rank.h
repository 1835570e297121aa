// What the rank entries of the grouped family share (rank.hip, rank_exclude.hip, nearest.hip, rank_bf16.hip, where_rank.hip,
// where_rank_bf16.hip): ONE row post-pass (rk_post) under a score policy per table format, ONE main-kernel skeleton over the
// fp32 table (rk_rank_body) with its two candidate streams, and on the host one checked start (rk_begin) and one D x BIAS
// dispatch (rk_dispatch).  The __global__ kernels stay in their units under their own names, launch bounds and
// amdgpu_waves_per_eu: each is a wrapper around a body here.  The score chains are rank_chain.h's and rank_chain_bf16.h's, the
// predicate and its count where_rank.h's.  The main kernels over the bf16 copy (rb_rank_kernel, wrb_rank_kernel) keep their
// own text in their units: their chunk pipeline differs on purpose (rk_chain replaces the lane's row registers step by step
// while it scores, the bf16 stream copies bn), and a shared bf16 skeleton measured slower.
#pragma once
#include "common.h"
#include "grouped_select.h"        // the item decode, the tile load, the dispatch on a tile's row groups; rg_better
#include "rank_chain.h"
#include "rank_chain_bf16.h"
#include "where_rank.h"

// ---- the row post-pass -----------------------------------------------------------------------------------------------------
// A score policy: the one-row query image in LDS (Image), its fill (row 0 the row's proj, rows 1..15 zero: an MFMA's output
// row depends on its own A row alone) and the score of the lanes' 16 columns against it through the unit's chain (the
// dimensions in index order), so g and every s_e are the bits the main kernel compared.  id < 0: a column without a product.
template <int D>
struct RkScoreF32 {
    using Table = float;
    using Image = float[16 * RK_QS(D)];
    static __device__ __forceinline__ void fill(Image& q, const float* __restrict__ row, int lane) {
        constexpr int QS = RK_QS(D);
        for (int e = lane; e < 16 * (QS / 4); e += 64) {
            const int r = e / (QS / 4), d4 = e - r * (QS / 4);
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r == 0 && d4 < D / 4) x = reinterpret_cast<const float4*>(row)[d4];
            *reinterpret_cast<float4*>(&q[r * QS + 4 * d4]) = x;
        }
    }
    static __device__ __forceinline__ float score(const Image& q, const float* __restrict__ table, int id, int c, int h) {
        float4 b[D / 16];                                 // (a lane without a product reads product 0's row: nothing of it is used)
        const float4* f = reinterpret_cast<const float4*>(table + (size_t)max(id, 0) * D) + h;
#pragma unroll
        for (int k = 0; k < D / 16; k++) b[k] = f[4 * k];
        f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
        rk_chain<D, 1>(q, 0, b, nullptr, acc, c, h);
        // C/D map of the 16x16 f32 MFMA: column lane & 15, row 4 (lane >> 4) + reg: row 0 is register 0 of lanes 0..15
        return acc[0][0];
    }
};

template <int D>
struct RkScoreBf16 {
    using Table = uint16_t;
    using Image = bf16x8[3][(D / 8) * 16];                // the pieces p0, p1, p2 (split3)
    static __device__ __forceinline__ void fill(Image& q, const float* __restrict__ row, int lane) {
        for (int e = lane; e < 16 * (D / 8); e += 64) {
            const int d8 = e >> 4, r = e & 15;
            float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
            if (r == 0) {
                const float4* f = reinterpret_cast<const float4*>(row) + 2 * d8;
                x0 = f[0];
                x1 = f[1];
            }
            const Split3 sp = split3(x0, x1);
            q[0][d8 * 16 + r] = sp.p0;
            q[1][d8 * 16 + r] = sp.p1;
            q[2][d8 * 16 + r] = sp.p2;
        }
    }
    static __device__ __forceinline__ float score(const Image& q, const uint16_t* __restrict__ table, int id, int c, int h) {
        bf16x8 b[D / 32];
        rb_load_b<D>(b, table, id, h);
        f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
        rb_chain<D, 16, 1>(q, 0, b, acc, c, h);
        return acc[0][0];                                 // (the 16x16 MFMAs' C/D map: row 0 is register 0 of lanes 0..15)
    }
};

// THE row post-pass, one wave per row (blockIdx.x), after the main kernel on the stream: every slice's atomic has landed.  The
// main kernel counted over the whole type (WHERE: over the products that pass the row's predicate); this takes the row's
// excluded products out again.  The B operand is blocks of 16 columns -- column 0 of the first block the target y, then the
// row's list ex_col[elo, elo + len).  A list entry e with cand_type[e] == types[r] (WHERE: that passes the predicate -- a failing
// entry was never counted) and rg_better(s_e, e, g, y) was counted: one off.  e == y, or cand_type[y] != types[r]: the target is
// no candidate of the row, rank -1; WHERE: a target that fails its own row's predicate too.  A row the plan left at -1 stays so;
// an id outside [0, num_products) is passed over; a key outside [-1, n_keys) is no list and is counted in *bad_count.  Without
// WHERE the kernel runs with lists only and the key is read unconditionally; with it the kernel runs in every call and the list
// part hangs on row_key (wave-uniform).  BIAS: s = fl(d + bias[id]), the main kernel's one addition.  Integer work, the row's
// wave the one writer.
template <int D, class Score, bool BIAS, bool WHERE>
__device__ __forceinline__ void rk_post(typename Score::Image& q, const float* __restrict__ proj, const int32_t* __restrict__ types,
                                        const int32_t* __restrict__ targets, const int32_t* __restrict__ row_key,
                                        const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col, int n_keys,
                                        const int32_t* __restrict__ cand_type, const typename Score::Table* __restrict__ table,
                                        const float* __restrict__ bias, int num_products, const pc_row_where& wh,
                                        int32_t* __restrict__ rank_out, int32_t* __restrict__ bad_count) {
    const int lane = threadIdx.x, c = lane & 15, h = lane >> 4;
    const int r = blockIdx.x;
    const bool lists = !WHERE || row_key;
    int key = -1;
    if (lists) {
        key = row_key[r];
        if (key < -1 || key >= n_keys) {
            if (lane == 0) atomicAdd(bad_count, 1);
            key = -1;
        }
    }
    const int base = rank_out[r];
    if (base < 0) return;                                 // (wave-uniform, as every exit below) no type, or an id out of range
    const int t = types[r], y = targets[r];               // both inside their ranges: the plan counted the row
    WrRow w{};
    bool out = lists && cand_type[y] != t;
    if constexpr (WHERE) {
        w = wr_row(wh, r);
        out = out || !wr_pass(w, wr_value(wh, y), wr_flags(wh, y));
    }
    if (out) {
        if (lane == 0) rank_out[r] = -1;
        return;
    }
    if (key < 0) return;
    const int elo = ex_rowptr[key], len = ex_rowptr[key + 1] - elo;
    if (len <= 0) return;
    Score::fill(q, proj + (size_t)r * D, lane);
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
        float bs = 0.f;
        if constexpr (BIAS) bs = bias[max(id, 0)];
        bool ok = true;
        if constexpr (WHERE) ok = wr_pass(w, wr_value(wh, id), wr_flags(wh, id));
        const float d = Score::score(q, table, id, c, h);
        const float s = BIAS ? d + bs : d;
        if (v0 == 0) g = __shfl(s, 0, 64);
        const bool mine = h == 0 && v > 0 && id >= 0;
        hit |= __any(mine && id == y);
        dec += __popcll(__ballot(mine && id != y && ok && cand_type[max(id, 0)] == t && rg_better(s, id, g, y)));
    }
    if (lane == 0) rank_out[r] = hit ? -1 : base - dec;
}

// ---- the main kernel over the fp32 table -------------------------------------------------------------------------------------
// f(integral_constant<NG>) for the NG in [1, RG] that equals rg (rg_dispatch_groups, in the rank kernels' order: the small
// tiles first).
template <int RG, class F>
__device__ __forceinline__ void rk_dispatch_groups(int rg, F& f) {
    if (rg == 1) f(std::integral_constant<int, 1>{});
    else if (rg == 2) f(std::integral_constant<int, 2>{});
    else if constexpr (RG == 4) {
        if (rg == 3) f(std::integral_constant<int, 3>{});
        else f(std::integral_constant<int, 4>{});
    }
}

// One work item's candidate stream for a tile of NG 16-row groups (NG a template argument: the loop body is straight-line
// code).  Lane l of wave wv: column c = l & 15 (candidate wv * 16 + c of the chunk, query row g * 16 + c of the A operand),
// k-lane h = l >> 4; accumulator register k of row group g holds query row g * 16 + 4 h + k.  b / pid / bs: the first chunk's
// rows, product ids and terms, pidn: the second chunk's ids, all already in flight (-1: a column past the slice's end; its b is
// product 0's row, its term bias[0], and its scores are not counted).  Leaves the wave's counts in part[wv][row].
template <int D, int NG, bool BIAS>
__device__ __forceinline__ void rk_stream(const float* q, const float* gs, const int* ys, int (*part)[8192 / D],
                                          const int32_t* __restrict__ type_col, const float* __restrict__ table,
                                          const float* __restrict__ bias, int cb0, int ce, float4 (&b)[D / 16], int pid, int pidn,
                                          float bs, int wv, int c, int h) {
    float gv[NG][4];
    int cn[NG][4];
#pragma unroll
    for (int g = 0; g < NG; g++) {
        const float4 x = *reinterpret_cast<const float4*>(&gs[g * 16 + 4 * h]);
        gv[g][0] = x.x; gv[g][1] = x.y; gv[g][2] = x.z; gv[g][3] = x.w;
#pragma unroll
        for (int k = 0; k < 4; k++) cn[g][k] = 0;
    }
    for (int cb = cb0; cb < ce; cb += RG_CHUNK) {
        const int cc = cb + 2 * RG_CHUNK + wv * 16 + c;
        const int pidnn = cc < ce ? type_col[cc] : -1;
        // the next chunk's rows replace this one's step by step while it is scored
        const float4* next = reinterpret_cast<const float4*>(table + (size_t)max(pidn, 0) * D) + h;
        f32x4 acc[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        rk_chain<D, NG>(q, 0, b, next, acc, c, h);
        // a score (BIAS: s = fl(d + bias[pid]), the one addition) above g is counted.  Equal to g (the target itself, a copy of
        // its row, or chance): the product index decides -- rare, so the rows' targets stay in LDS and are read only where a
        // lane meets such a score
        if (pid >= 0) {
            bool tie = false;
#pragma unroll
            for (int g = 0; g < NG; g++) {
                if constexpr (BIAS) acc[g] += bs;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    cn[g][k] += acc[g][k] > gv[g][k] ? 1 : 0;
                    tie |= acc[g][k] == gv[g][k];
                }
            }
            if (tie) {
#pragma unroll
                for (int g = 0; g < NG; g++)
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        cn[g][k] += (acc[g][k] == gv[g][k] && pid < ys[g * 16 + 4 * h + k]) ? 1 : 0;
            }
        }
        if constexpr (BIAS) bs = bias[max(pidn, 0)];      // the next chunk's term, with its product id, a chunk ahead
        pid = pidn;
        pidn = pidnn;
    }
    wr_reduce<NG, 8192 / D>(cn, part, wv, c, h);          // the 16 columns of a (wave, k-lane) -> lane c == 0 -> part[wv][row]
}

// rk_stream with the test in the count: gs / ys / wq: the rows' target scores, targets and predicates; a / f: the first
// chunk's attributes (a column past the slice's end: entry 0's, and nothing of it is counted).
template <int D, int NG, bool BIAS>
__device__ __forceinline__ void wr_stream(const float* q, const float* gs, const int* ys, const WrRow* wq, int (*part)[8192 / D],
                                          const int32_t* __restrict__ type_col, const float* __restrict__ table,
                                          const float* __restrict__ bias, const pc_row_where& wh, int cb0, int ce,
                                          float4 (&b)[D / 16], int pid, int pidn, float bs, float a, int f, int wv, int c, int h) {
    int cn[NG][4];
#pragma unroll
    for (int g = 0; g < NG; g++)
#pragma unroll
        for (int k = 0; k < 4; k++) cn[g][k] = 0;
    for (int cb = cb0; cb < ce; cb += RG_CHUNK) {
        const int cc = cb + 2 * RG_CHUNK + wv * 16 + c;
        const int pidnn = cc < ce ? type_col[cc] : -1;
        // the next chunk's rows replace this one's step by step while it is scored
        const float4* next = reinterpret_cast<const float4*>(table + (size_t)max(pidn, 0) * D) + h;
        f32x4 acc[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        rk_chain<D, NG>(q, 0, b, next, acc, c, h);
        wr_count<NG, BIAS>(acc, bs, gs, cn, ys, wq, pid, a, f, h);
        // the next chunk's term and attributes, with its product id, a chunk ahead
        if constexpr (BIAS) bs = bias[max(pidn, 0)];
        a = wr_value(wh, pidn);
        f = wr_flags(wh, pidn);
        pid = pidn;
        pidn = pidnn;
    }
    wr_reduce<NG, 8192 / D>(cn, part, wv, c, h);
}

// THE skeleton of rk_rank_kernel, nb_rank_kernel (BIAS) and wr_rank_kernel (WHERE): grid-stride over the work items
// w = (type t, slice s, tile j), items of one type ordered slice-major so that the tiles running side by side read the same
// candidates (L2): query tile -> LDS; the first two chunks in flight; the tile's own targets scored on the MFMA diagonal into
// gs / ys (g = d(r, y), BIAS: + bias[y]); WHERE: the rows' lo / hi / need / deny read through order[p0 + row] once per work item
// into LDS beside them, value[pid] / flags[pid] gathered a chunk ahead with the product id; then the slice's candidates against
// the tile's NG row groups, straight-line code per NG; the four waves' counts through LDS into one integer atomic per
// (row, slice).  wh is read under WHERE alone.
template <int D, bool BIAS, bool WHERE>
__device__ __forceinline__ void rk_rank_body(const float* __restrict__ proj, const int32_t* __restrict__ targets,
                                             const int32_t* __restrict__ type_rowptr, const int32_t* __restrict__ type_col,
                                             const float* __restrict__ table, const float* __restrict__ bias, int n_types, int S,
                                             const int32_t* __restrict__ cnt, const int32_t* __restrict__ row_start,
                                             const int64_t* __restrict__ item_start, const int32_t* __restrict__ order,
                                             int32_t* __restrict__ rank_out, const pc_row_where& wh) {
    constexpr int TM = 8192 / D;             // rows per tile: 64 (D = 128) or 32 (D = 256): a 32 KB query tile
    constexpr int RG = TM / 16;              // 16-row groups (at most one per wave)
    constexpr int QS = RK_QS(D);             // padded LDS row
    constexpr int NB = D / 16;               // float4 operands per lane per candidate
    __shared__ __attribute__((aligned(16))) float q[TM * QS];
    __shared__ __attribute__((aligned(16))) float gs[TM];            // the rows' target scores
    __shared__ __attribute__((aligned(16))) int ys[TM];              // the rows' targets
    __shared__ WrRow wq[WHERE ? TM : 1];                             // the rows' predicates (WHERE alone: never touched without)
    __shared__ int part[4][TM];                                      // the waves' counts
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, h = lane >> 4;
    const int64_t n_items = item_start[n_types];
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const RgItem it = rg_decode<TM>(w, item_start, cnt, row_start, type_rowptr, n_types, S);
        const int p0 = it.p0, valid = it.valid, rg = it.rg, cb0 = it.cb0, ce = it.ce;

        __syncthreads();                                  // the previous item's readers of q / wq / part are done
        rg_load_tile<D, QS>(q, proj, order, p0, valid, rg, tid);
        if constexpr (WHERE) {
            if (tid < TM) wq[tid] = wr_row(wh, tid < valid ? order[p0 + tid] : -1);
        }

        auto load_pid = [&](int cb) { const int cc = cb + wv * 16 + c; return cc < ce ? type_col[cc] : -1; };
        // (a lane without a product reads product 0's row, term and attributes: no branch, and nothing of it is used)
        auto load_b = [&](float4* b, int pid) {
            const float4* f = reinterpret_cast<const float4*>(table + (size_t)max(pid, 0) * D) + h;
#pragma unroll
            for (int k = 0; k < NB; k++) b[k] = f[4 * k];
        };
        float4 b[NB];
        const int pid = load_pid(cb0);
        load_b(b, pid);
        float bs = 0.f, a = 0.f;
        int f = 0;
        if constexpr (BIAS) bs = bias[max(pid, 0)];
        if constexpr (WHERE) {
            a = wr_value(wh, pid);
            f = wr_flags(wh, pid);
        }
        const int pidn = load_pid(cb0 + RG_CHUNK);
        // wave wv: column c = the target of query row wv * 16 + c
        int ty = -1;
        if (wv < rg && wv * 16 + c < valid) ty = targets[order[p0 + wv * 16 + c]];
        __syncthreads();                                  // query tile in LDS
        if (wv < rg) {                                    // (wave-uniform)
            float4 bt[NB];
            load_b(bt, ty);
            float by = 0.f;
            if constexpr (BIAS) by = bias[max(ty, 0)];
            f32x4 ag[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
            rk_chain<D, 1>(q, wv, bt, nullptr, ag, c, h);
            const f32x4 acc = ag[0];
            // C/D map of the 16x16 f32 MFMA: column lane & 15, row 4 (lane >> 4) + reg; the diagonal: row == column
            if ((c >> 2) == h) {
                const int k = c & 3;
                const float d = k == 0 ? acc[0] : k == 1 ? acc[1] : k == 2 ? acc[2] : acc[3];
                gs[wv * 16 + c] = BIAS ? d + by : d;
                ys[wv * 16 + c] = ty;
            }
        }
        __syncthreads();                                  // gs / ys / wq in LDS
        auto stream = [&](auto groups) {
            constexpr int NG = decltype(groups)::value;
            if constexpr (WHERE)
                wr_stream<D, NG, BIAS>(q, gs, ys, wq, part, type_col, table, bias, wh, cb0, ce, b, pid, pidn, bs, a, f, wv, c, h);
            else
                rk_stream<D, NG, BIAS>(q, gs, ys, part, type_col, table, bias, cb0, ce, b, pid, pidn, bs, wv, c, h);
        };
        rk_dispatch_groups<RG>(rg, stream);
        __syncthreads();
        if (tid < valid) {
            const int v = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
            if (v) atomicAdd(&rank_out[order[p0 + tid]], v);
        }
    }
}

// ---- the entries on the host --------------------------------------------------------------------------------------------------
// THE checked start of a rank entry, the refusals in the entries' order: the pointers (args_ok: the entry's own -- proj, its
// table, a bias it cannot do without, its filter's pairing), the counts, the lists with the products' types (all or none) --
// PC_EINVAL; the shapes and, for a bf16 table, its 16-byte alignment (table16: null for an fp32 table) -- PC_ESHAPE; then the
// workspace (PC_EWORKSPACE), the plan's launches and the hot kernel's grid (rg_begin).
struct RkStart {
    RgWs w;
    unsigned grid;
    int S;
    hipStream_t st;
};
inline int rk_begin(RkStart& s, bool args_ok, const void* table16, const int32_t* types, const int32_t* targets,
                    const int32_t* row_key, int rows, const int32_t* type_rowptr, const int32_t* type_col, int n_types,
                    int num_products, const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, const int32_t* cand_type,
                    int dim, int slices, int32_t* rank_out, int32_t* bad_count, void* ws, size_t ws_bytes, void* stream) {
    if (!args_ok || !types || !targets || !type_rowptr || !type_col || !rank_out || !bad_count || !ws) return PC_EINVAL;
    if (rows <= 0 || n_types <= 0 || num_products <= 0) return PC_EINVAL;
    if (!rg_lists_ok(row_key, ex_rowptr, ex_col, bad_count, n_keys) || !row_key != !cand_type) return PC_EINVAL;
    if ((dim != 128 && dim != 256) || slices < 0 || slices > RG_MAX_SLICES) return PC_ESHAPE;
    if ((uintptr_t)table16 & 15) return PC_ESHAPE;        // a lane reads 16 bytes of a row at once
    s.S = rg_slices(slices);
    s.st = (hipStream_t)stream;
    return rg_begin(s.w, s.grid, ws, ws_bytes, types, targets, rows, type_rowptr, n_types, num_products, 0, s.S, 8192 / dim,
                    rank_out, bad_count, s.st);
}

// f(integral_constant<int, D>, bool_constant<BIAS>) for the entry's dim (128 or 256: checked) and bias; an entry whose kernels
// have no BIAS argument passes false and reads D alone.
template <class F>
inline void rk_dispatch(int dim, bool bias, F&& f) {
    if (dim == 128) {
        if (bias) f(std::integral_constant<int, 128>{}, std::true_type{});
        else f(std::integral_constant<int, 128>{}, std::false_type{});
    } else {
        if (bias) f(std::integral_constant<int, 256>{}, std::true_type{});
        else f(std::integral_constant<int, 256>{}, std::false_type{});
    }
}
