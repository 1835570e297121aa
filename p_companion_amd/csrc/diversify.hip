// Diversified lists: a greedy maximal-marginal-relevance re-rank of the served long lists on the device (pc_diversify_lists;
// ops.diversify_lists, PCompanionInference.recommend_diverse_batch), and the per-product factor that makes its similarity a
// cosine (pc_inv_norm).  The pool of a row is what pc_retrieve_list_grouped / pc_retrieve_topk_grouped return: idx / score
// [rows][m], m <= 256, in any order, -1 ids and non-finite scores anywhere.  The output is the n <= m products to show, in pick
// order, each with its INPUT score.
//
//   similarity   sim(a, b) = fl(d(a, b) * fl(scale[a] * scale[b])), without a scale d(a, b); d = dv_dot below, ONE device
//                function for every variant: the fp32 dot product of the two table rows as four fused-multiply-add chains from
//                zero -- chain e takes the dimensions 4 k + e of the lane's 128-dimension part, k ascending -- joined as
//                (c0 + c2) + (c1 + c3); at D = 256 the two 128-dimension parts of a slot live in adjacent lanes and their sums
//                meet in one addition.  Every operation is commutative in its two rows, so sim(a, b) = sim(b, a) bit for bit,
//                and the order is a function of the dimension index alone: a pair's bits do not depend on m, n, the slot, the
//                variant, the grid or the run.
//   round t      v_j = fl(lam * score_j) at t = 0, fl(fl(lam * score_j) - fl(mu * pen_j)) later, pen_j = the maximum of
//                sim(j, i) over the picks i so far; dv_value, contraction off: three roundings.  The pick is the best remaining
//                candidate under rg_better (value descending, product index ascending); among slots equal in (value, id) --
//                duplicate ids, outside the contract -- the lowest slot.
//   kernel       one workgroup per row, grid-stride.  Slot j belongs to D / 128 adjacent lanes, which hold their part of the
//                product's row, gathered from the table ONCE, in 32 float4 = 128 registers through the rounds.  The gather
//                goes through 16 staging rows per wave in LDS: 32 lanes fetch a lane's 512 bytes together (16-byte loads, two
//                whole parts per wave instruction), and each lane reads its row back.  (A lane fetching its own 512 bytes, 64
//                rows per wave instruction, measured 1.0 ms for the 1.6 GB of 12 288 pools of 256 at 10 M products; staged,
//                0.29 ms.)  Per round: the wave's best (shuffle tree) and its first holder (ballot) -> LDS, barrier, every thread
//                folds the waves' bests in wave order; the picked slot's lanes copy their registers to an LDS row, barrier,
//                every live lane reads that row (one address per part: a broadcast) and adds one chain to its running
//                maximum.  Two barriers per round.  The picks collect in LDS and leave as coalesced stores at the row's end.
//   variants     CAP = 64 slots (m <= 64: one wave at D = 128, two at D = 256) and CAP = 256 (four / eight waves).  D = 256
//                takes a second lane per slot rather than 256 registers per lane (which leaves no register for anything else
//                without the accumulation file) or a re-read of the pool's rows through L2 in every round (n times the
//                gather's bytes): a lane's registers and code are those of D = 128.
//   bf16 table   pc_diversify_lists_bf16 / pc_inv_norm_bf16 read the [P, D] bf16 copy of the catalogue (ops.CompactCatalogue)
//                and return, bit for bit, what the fp32 entries return on the widened table: widening bf16 -> fp32 is exact,
//                and everything after the gather -- dv_dot, dv_sim, dv_value, the pick rule, the norm's summation order -- is
//                the same code on the same fp32 registers.  The kernels are templated on the table's element type; only the
//                gather differs.  A lane's part is 256 bytes: 16 lanes fetch it together (16-byte loads, FOUR whole parts per
//                wave instruction), the bf16 patterns are staged in the same per-wave LDS rows -- two parts side by side in a
//                row, so 32 lanes' parts per pass and as many loads in flight as the fp32 gather has -- and widened at the
//                read-back.
// No workspace, no float atomics (one integer atomic per id out of range), nothing read back.
#include "common.h"
#include "grouped_select.h"        // rg_better, RG_NONE, RG_MAX_GRID

#define DV_MAX_POOL 256
#define DV_PART 128                // dimensions per lane
#define DV_NB (DV_PART / 4)        // float4 registers per lane
#define DV_ST (DV_PART + 4)        // a staging row in LDS, padded: 16 lanes read 16 rows without a bank conflict

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// bf16 -> fp32, exact: the pattern is the upper half of the fp32 pattern.  Two packed elements: the lower address in the low half.
__device__ __forceinline__ float dv_widen_lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float dv_widen_hi(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }

// The dot product of a lane's part x of its slot's row with the same part of the picked row (LDS, every lane of a part reads
// the same address), then the parts' sums.  LPS = D / 128 lanes per slot, adjacent.  The four chains are written as two
// two-wide fused multiply-adds over the register pairs as they lie (x.xy, x.zw): left to itself the vectoriser pairs the
// chains (c1, c3) / (c0, c2) and keeps a second, shuffled copy of the lane's 128 registers for it.
template <int LPS>
__device__ __forceinline__ float dv_dot(const f32x4 (&x)[DV_NB], const float* __restrict__ prow_part) {
    f32x2 c01 = {0.f, 0.f}, c23 = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < DV_NB; k++) {
        const f32x4 y = *reinterpret_cast<const f32x4*>(prow_part + 4 * k);
        c01 = __builtin_elementwise_fma(x[k].xy, y.xy, c01);
        c23 = __builtin_elementwise_fma(x[k].zw, y.zw, c23);
    }
    const f32x2 c = c01 + c23;                            // (c0 + c2, c1 + c3)
    float s = c.x + c.y;
    if constexpr (LPS == 2) s = s + __shfl_xor(s, 1, 64);                // (a + b = b + a: both lanes hold the same bits)
    return s;
}

// sim(a, b): the chain times the rounded product of the two factors (a product of two floats commutes)
__device__ __forceinline__ float dv_sim(float d, bool scaled, float sa, float sb) {
#pragma clang fp contract(off)
    const float f = sa * sb;
    return scaled ? d * f : d;
}

// A candidate's value in round t: fl(lam * score) at t = 0 (ls), fl(ls - fl(mu * pen)) later.  Contraction is off: the product
// and the difference round separately, as documented (the headers' __fmul_rn / __fsub_rn are plain operators and would fuse).
__device__ __forceinline__ float dv_scaled_score(float lam, float sc) {
#pragma clang fp contract(off)
    return lam * sc;
}
__device__ __forceinline__ float dv_value(float ls, float mu, float pen, bool first) {
#pragma clang fp contract(off)
    const float q = mu * pen;
    const float v = first ? ls : ls - q;
    return v == v ? v : -INFINITY;                        // (a NaN -- a non-finite table row -- ranks last, not nowhere)
}

// CAP slots, LPS lanes per slot: CAP * LPS threads.  mu = fl(1 - lam), formed on the host.  T: the table's element type, float
// or uint16_t (bf16 patterns).
template <int D, int CAP, typename T>
__global__ __launch_bounds__(CAP * (D / DV_PART)) void dv_mmr_kernel(const int32_t* __restrict__ idx,
                                                                     const float* __restrict__ score, int rows, int m,
                                                                     const T* __restrict__ table,
                                                                     const float* __restrict__ scale, int num_products, int n,
                                                                     float lam, float mu, int32_t* __restrict__ out_idx,
                                                                     float* __restrict__ out_score,
                                                                     int32_t* __restrict__ bad_count) {
    constexpr int LPS = D / DV_PART, NT = CAP * LPS, NW = NT / 64;
    __shared__ __attribute__((aligned(16))) float prow[D];           // the picked product's row
    __shared__ float pscale;                                         // ... and its factor
    __shared__ __attribute__((aligned(16))) float stage[NW][16][DV_ST];     // the gather's staging rows, 16 per wave
    __shared__ float wv[NW];                                         // the waves' bests: value, product, slot
    __shared__ int wi[NW], wslot[NW];
    __shared__ int res_i[CAP];                                       // the row's picks
    __shared__ float res_s[CAP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = tid / LPS, part = tid % LPS;
    const bool scaled = scale != nullptr;
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        __syncthreads();                                  // the previous row's picks have left res_i / res_s
        // ---- the slot's candidate: id, score, factor, its part of the table row
        int pid = RG_NONE;                                // RG_NONE: no candidate (or picked)
        float sc = 0.f;
        if (slot < m) {
            const int id = idx[(size_t)r * m + slot];
            const float s = score[(size_t)r * m + slot];
            if (id < -1 || id >= num_products) {          // never dereferenced
                if (bad_count && part == 0) atomicAdd(bad_count, 1);
            } else if (id >= 0 && __builtin_isfinite(s)) {
                pid = id;
                sc = s;
            }
        }
        // (a lane without a candidate reads product 0's row and factor -- no branch around 32 loads, and nothing of it is
        // used: the lane is never picked, and its running maximum is never read)
        const int row = pid == RG_NONE ? 0 : pid;
        const float sa = scaled ? scale[row] : 1.f;
        // The gather, through the wave's staging rows: a lane's 512 bytes are fetched by 32 lanes at once (a wave instruction
        // reads two whole parts, 1 KB, not 16 bytes of 64 different rows), 16 lanes' parts per pass, and come back from LDS
        // one row per lane.  Same-wave LDS instructions execute in order: no barrier between the store and the read-back.
        f32x4 x[DV_NB];
        if constexpr (std::is_same<T, float>::value) {
            float(*st)[DV_ST] = stage[wave];
            const int half = lane >> 5, chunk = lane & 31;
#pragma unroll
            for (int p = 0; p < 4; p++) {
                f32x4 y[8];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int owner = 16 * p + 2 * i + half;                  // the lane whose part this is (64 % LPS == 0)
                    const int orow = __shfl(row, owner, 64);
                    y[i] = *reinterpret_cast<const f32x4*>(table + (size_t)orow * D + (owner % LPS) * DV_PART + 4 * chunk);
                }
#pragma unroll
                for (int i = 0; i < 8; i++) *reinterpret_cast<f32x4*>(&st[2 * i + half][4 * chunk]) = y[i];
                __builtin_amdgcn_wave_barrier();
                const bool mine = (lane >> 4) == p;
#pragma unroll
                for (int k = 0; k < DV_NB; k++) {
                    const f32x4 z = *reinterpret_cast<const f32x4*>(&st[lane & 15][4 * k]);
                    x[k] = (mine || p == 0) ? z : x[k];
                }
                __builtin_amdgcn_wave_barrier();
            }
        } else {
            // bf16: a part is 256 bytes, fetched by 16 lanes at once (a wave instruction reads four whole parts); staging row
            // o & 15 holds the parts of the pass's owners o and o + 16 side by side (2 x 256 of its 528 bytes), so a pass
            // serves 32 lanes.  A lane reads its part back as 16 operands of 8 bf16 and widens them: x[k] holds the dimensions
            // 4 k .. 4 k + 3 of the part, as from the fp32 table.
            float(*st)[DV_ST] = stage[wave];
            const int quarter = lane >> 4, chunk = lane & 15;
#pragma unroll
            for (int p = 0; p < 2; p++) {
                u32x4 y[8];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int owner = 32 * p + 4 * i + quarter;                 // the lane whose part this is (64 % LPS == 0)
                    const int orow = __shfl(row, owner, 64);
                    y[i] = *reinterpret_cast<const u32x4*>(table + (size_t)orow * D + (owner % LPS) * DV_PART + 8 * chunk);
                }
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int o = 4 * i + quarter;                              // the owner within the pass: row o & 15, half o >> 4
                    *reinterpret_cast<u32x4*>(&st[o & 15][64 * (o >> 4) + 4 * chunk]) = y[i];
                }
                __builtin_amdgcn_wave_barrier();
                if ((lane >> 5) == p) {                   // (every lane belongs to exactly one pass: x is written once)
#pragma unroll
                    for (int k = 0; k < DV_NB / 2; k++) {
                        const u32x4 z = *reinterpret_cast<const u32x4*>(&st[lane & 15][64 * ((lane >> 4) & 1) + 4 * k]);
                        x[2 * k] = f32x4{dv_widen_lo(z.x), dv_widen_hi(z.x), dv_widen_lo(z.y), dv_widen_hi(z.y)};
                        x[2 * k + 1] = f32x4{dv_widen_lo(z.z), dv_widen_hi(z.z), dv_widen_lo(z.w), dv_widen_hi(z.w)};
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        for (int k = tid; k < n; k += NT) { res_i[k] = -1; res_s[k] = -INFINITY; }
        const float ls = dv_scaled_score(lam, sc);
        float pen = -INFINITY;
        for (int t = 0; t < n; t++) {
            // ---- the best remaining candidate: wave, then workgroup
            const float v = dv_value(ls, mu, pen, t == 0);
            float bv = pid == RG_NONE ? -INFINITY : v;
            int bi = pid;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (rg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            // its first holder in the wave (the lanes of a slot are adjacent: part 0 comes first)
            const unsigned long long holders = __ballot(pid != RG_NONE && pid == bi && v == bv);
            if (lane == 0) {
                wv[wave] = bv;
                wi[wave] = bi;
                wslot[wave] = holders ? (wave * 64 + (int)__builtin_ctzll(holders)) / LPS : -1;
            }
            __syncthreads();                              // A: the waves' bests (and, at t = 0, the cleared picks) are in LDS
            float gv = wv[0];
            int gi = wi[0], gslot = wslot[0];
#pragma unroll
            for (int w = 1; w < NW; w++) {                // (ties between waves: the lower wave, so the lower slot)
                const float ov = wv[w];
                const int oi = wi[w];
                if (rg_better(ov, oi, gv, gi)) { gv = ov; gi = oi; gslot = wslot[w]; }
            }
            if (gi == RG_NONE || gslot < 0) break;        // (uniform) the pool is exhausted: the rest stays -1 / -inf
            if (slot == gslot) {
                if (part == 0) { res_i[t] = pid; res_s[t] = sc; pscale = sa; }
                if (t + 1 < n) {
#pragma unroll
                    for (int k = 0; k < DV_NB; k++) *reinterpret_cast<f32x4*>(&prow[part * DV_PART + 4 * k]) = x[k];
                }
                pid = RG_NONE;                            // retired
            }
            if (t + 1 == n) break;                        // (uniform)
            __syncthreads();                              // B: the picked row is in LDS; wv / wi / wslot have been read
            if (__ballot(pid != RG_NONE)) {               // (wave-uniform: a wave without a live slot skips the chain)
                const float d = dv_dot<LPS>(x, prow + part * DV_PART);
                const float s = dv_sim(d, scaled, sa, pscale);
                pen = fmaxf(pen, s);
            }
        }
        __syncthreads();                                  // the picks are in LDS
        for (int k = tid; k < n; k += NT) {
            out_idx[(size_t)r * n + k] = res_i[k];
            out_score[(size_t)r * n + k] = res_s[k];
        }
    }
}

// out[p] = 1 / sqrt(sum_d e[p][d]^2), 0 for an all-zero row.  nb_half_sq_norm_kernel's sum (nearest.hip), restated: a group of
// 16 lanes owns a row; lane l of the group adds, in this order, the squares of the elements x, y, z, w of the float4s l, l + 16,
// .. (dimensions 4 l + 64 j + e, j ascending, e ascending) into one fp32 sum by fused multiply-add, starting from zero; the 16
// sums meet in a butterfly over the lane distances 8, 4, 2, 1 (every lane of the group holds the same bits).  Then one
// correctly rounded square root and one correctly rounded division.  No atomics; a row's value does not depend on the grid.
// T = uint16_t: the same four dimensions are 8 bytes of bf16 patterns, widened (exactly) before the sum.
template <int D, typename T>
__global__ __launch_bounds__(256) void dv_inv_norm_kernel(const T* __restrict__ table, int rows, float* __restrict__ out) {
    const int l = threadIdx.x & 15;
    const int64_t stride = (int64_t)gridDim.x * 16;
    for (int64_t p = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); p < rows; p += stride) {
        float4 x[D / 64];
        if constexpr (std::is_same<T, float>::value) {
            const float4* f = reinterpret_cast<const float4*>(table + (size_t)p * D) + l;
#pragma unroll
            for (int j = 0; j < D / 64; j++) x[j] = f[16 * j];
        } else {
            const u32x2* f = reinterpret_cast<const u32x2*>(table + (size_t)p * D) + l;
#pragma unroll
            for (int j = 0; j < D / 64; j++) {
                const u32x2 z = f[16 * j];
                x[j] = make_float4(dv_widen_lo(z.x), dv_widen_hi(z.x), dv_widen_lo(z.y), dv_widen_hi(z.y));
            }
        }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < D / 64; j++) {
            s = __builtin_fmaf(x[j].x, x[j].x, s);
            s = __builtin_fmaf(x[j].y, x[j].y, s);
            s = __builtin_fmaf(x[j].z, x[j].z, s);
            s = __builtin_fmaf(x[j].w, x[j].w, s);
        }
        // (a group's 16 lanes run the same number of iterations: p depends on threadIdx.x >> 4 alone)
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if (l == 0) out[p] = s == 0.f ? 0.f : 1.0f / sqrtf(s);      // (this build rounds both correctly: hipcc's default)
    }
}

namespace {
template <typename T>
int dv_inv_norm(const T* table, int rows, int dim, float* out, void* stream) {
    if (!table || !out || rows <= 0) return PC_EINVAL;
    if ((dim != 128 && dim != 256) || ((uintptr_t)table & 15)) return PC_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)min((rows + 15) / 16, RG_MAX_GRID));        // 16 rows per workgroup and pass, grid-stride
    if (dim == 128) PC_LAUNCH((dv_inv_norm_kernel<128, T>), grid, dim3(256), 0, st, table, rows, out);
    else PC_LAUNCH((dv_inv_norm_kernel<256, T>), grid, dim3(256), 0, st, table, rows, out);
    return pc_launch_status();
}

template <typename T>
int dv_diversify(const int32_t* idx, const float* score, int rows, int m, const T* table, const float* scale, int num_products,
                 int dim, int n, float lam, int32_t* out_idx, float* out_score, int32_t* bad_count, void* stream) {
    if (rows < 0 || m < 1 || m > DV_MAX_POOL || n < 1 || n > m || (dim != 128 && dim != 256) || num_products < 1) return PC_ESHAPE;
    if (!(lam >= 0.f && lam <= 1.f)) return PC_ESHAPE;                     // (a NaN fails both comparisons)
    if (rows == 0) return PC_OK;                                          // nothing to serve: no launch, no pointer is read
    if (!idx || !score || !table || !out_idx || !out_score || ((uintptr_t)table & 15)) return PC_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const float mu = 1.0f - lam;                                          // fl(1 - lam)
    const dim3 grid((unsigned)min(rows, RG_MAX_GRID));                    // one row per workgroup and pass: never more than rows
#define DV_MMR(D, CAP)                                                                                                          \
    PC_LAUNCH((dv_mmr_kernel<D, CAP, T>), grid, dim3(CAP * (D / DV_PART)), 0, st, idx, score, rows, m, table, scale,            \
              num_products, n, lam, mu, out_idx, out_score, bad_count)
    if (dim == 128) {
        if (m <= 64) DV_MMR(128, 64); else DV_MMR(128, 256);
    } else {
        if (m <= 64) DV_MMR(256, 64); else DV_MMR(256, 256);
    }
#undef DV_MMR
    return pc_launch_status();
}
}  // namespace

extern "C" int pc_inv_norm(const float* table, int rows, int dim, float* out, void* stream) {
    return dv_inv_norm(table, rows, dim, out, stream);
}

extern "C" int pc_inv_norm_bf16(const uint16_t* table_bf16, int rows, int dim, float* out, void* stream) {
    return dv_inv_norm(table_bf16, rows, dim, out, stream);
}

extern "C" int pc_diversify_lists(const int32_t* idx, const float* score, int rows, int m, const float* table, const float* scale,
                                  int num_products, int dim, int n, float lam, int32_t* out_idx, float* out_score,
                                  int32_t* bad_count, void* stream) {
    return dv_diversify(idx, score, rows, m, table, scale, num_products, dim, n, lam, out_idx, out_score, bad_count, stream);
}

extern "C" int pc_diversify_lists_bf16(const int32_t* idx, const float* score, int rows, int m, const uint16_t* table_bf16,
                                       const float* scale, int num_products, int dim, int n, float lam, int32_t* out_idx,
                                       float* out_score, int32_t* bad_count, void* stream) {
    return dv_diversify(idx, score, rows, m, table_bf16, scale, num_products, dim, n, lam, out_idx, out_score, bad_count, stream);
}
