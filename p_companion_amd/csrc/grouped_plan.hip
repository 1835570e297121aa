// The planning launches of the type-grouped catalogue kernels (grouped_plan.h; every entry of the family calls them) and the
// host plumbing of the entries:
//   count   pos[r] = atomic position of row r among the rows of its type, cnt[t] = rows of type t
//   scan    (one workgroup) row_start[t] = exclusive sum of cnt, item_start[t] = exclusive sum of tiles(t) * slices(t)
//   place   order[row_start[t] + pos[r]] = r
// The order of the rows inside a type is the one thing the atomics decide; nothing the callers return depends on it.
#include "grouped_plan.h"

// pos[r] < 0: the row takes no part.
__global__ __launch_bounds__(256) void rg_count_kernel(const int32_t* __restrict__ types, const int32_t* __restrict__ targets,
                                                       int rows, int n_types, int num_products, int32_t* __restrict__ cnt,
                                                       int32_t* __restrict__ pos, int32_t* __restrict__ rank_out,
                                                       int32_t* __restrict__ bad_count) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int t = types[r];
    int p = -1;
    if (t >= 0) {                                         // (t < 0: no type matched -- skipped, not an error)
        bool ok = t < n_types;
        if (ok && targets) { const int y = targets[r]; ok = y >= 0 && y < num_products; }
        if (ok) p = atomicAdd(&cnt[t], 1);
        else if (bad_count) atomicAdd(bad_count, 1);
    }
    pos[r] = p;
    if (rank_out) rank_out[r] = p < 0 ? -1 : 0;
}

// One workgroup: each thread sums a contiguous run of types, a block scan of the run totals, then the run is written.
__global__ __launch_bounds__(1024) void rg_scan_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ type_rowptr,
                                                       int n_types, int S, int TM, int32_t* __restrict__ row_start,
                                                       int64_t* __restrict__ item_start) {
    __shared__ int64_t sr[1024], si[1024];
    const int tid = threadIdx.x;
    const int per = (n_types + 1023) / 1024;
    const int t0 = min(tid * per, n_types), t1 = min(t0 + per, n_types);
    auto items = [&](int t, int c) -> int64_t {
        int ns, L;
        rg_slice_plan(type_rowptr[t + 1] - type_rowptr[t], S, ns, L);
        return c > 0 ? (int64_t)((c + TM - 1) / TM) * ns : 0;
    };
    int64_t a = 0, b = 0;
    for (int t = t0; t < t1; t++) { const int c = cnt[t]; a += c; b += items(t, c); }
    sr[tid] = a; si[tid] = b;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                  // inclusive Hillis-Steele scan
        const int64_t xa = tid >= o ? sr[tid - o] : 0, xb = tid >= o ? si[tid - o] : 0;
        __syncthreads();
        sr[tid] += xa; si[tid] += xb;
        __syncthreads();
    }
    int64_t ra = sr[tid] - a, rb = si[tid] - b;
    for (int t = t0; t < t1; t++) {
        const int c = cnt[t];
        row_start[t] = (int32_t)ra; item_start[t] = rb;
        ra += c; rb += items(t, c);
    }
    if (tid == 1023) { row_start[n_types] = (int32_t)sr[1023]; item_start[n_types] = si[1023]; }
}

__global__ __launch_bounds__(256) void rg_place_kernel(const int32_t* __restrict__ types, int rows,
                                                       const int32_t* __restrict__ pos, const int32_t* __restrict__ row_start,
                                                       int32_t* __restrict__ order) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int p = pos[r];
    if (p >= 0) order[row_start[types[r]] + p] = r;       // (p >= 0 only for a type inside [0, n_types))
}

RgPlan rg_plan_carve(WsCarver& cv, int rows, int n_types) {
    RgPlan w;
    w.cnt = (int32_t*)cv.bytes((size_t)n_types * 4);
    w.pos = (int32_t*)cv.bytes((size_t)rows * 4);
    w.row_start = (int32_t*)cv.bytes((size_t)(n_types + 1) * 4);
    w.item_start = (int64_t*)cv.bytes((size_t)(n_types + 1) * 8);
    w.order = (int32_t*)cv.bytes((size_t)rows * 4);
    return w;
}

int rg_plan_launch(const RgPlan& w, const int32_t* types, const int32_t* targets, int rows, const int32_t* type_rowptr,
                   int n_types, int num_products, int S, int TM, int32_t* rank_out, int32_t* bad_count, hipStream_t st) {
    PC_HIP_TRY(hipMemsetAsync(w.cnt, 0, (size_t)n_types * 4, st));
    const dim3 rgrid((rows + 255) / 256);
    PC_LAUNCH(rg_count_kernel, rgrid, dim3(256), 0, st, types, targets, rows, n_types, num_products, w.cnt, w.pos, rank_out,
              bad_count);
    PC_LAUNCH(rg_scan_kernel, dim3(1), dim3(1024), 0, st, w.cnt, type_rowptr, n_types, S, TM, w.row_start, w.item_start);
    PC_LAUNCH(rg_place_kernel, rgrid, dim3(256), 0, st, types, rows, w.pos, w.row_start, w.order);
    return PC_OK;                                         // (the launches' status: the caller's pc_launch_status())
}

unsigned rg_item_grid(int rows, int n_types, int S, int TM) {
    const int64_t cap = ((int64_t)(rows + TM - 1) / TM + (int64_t)(rows < n_types ? rows : n_types)) * S;
    return (unsigned)(cap < RG_MAX_GRID ? cap : RG_MAX_GRID);
}

RgWs rg_ws_carve(void* ws, int rows, int n_types, int n, int S) {
    RgWs w;
    WsCarver cv(ws);
    w.plan = rg_plan_carve(cv, rows, n_types);
    w.pv = (float*)cv.bytes((size_t)rows * S * n * 4);
    w.pi = (int32_t*)cv.bytes((size_t)rows * S * n * 4);
    w.bytes = cv.total;
    return w;
}

size_t rg_topn_workspace_bytes(int rows, int n_types, int n, int max_n, int slices) {
    if (rows <= 0 || n_types <= 0 || n < 1 || n > max_n || slices < 0 || slices > RG_MAX_SLICES) return 0;
    return rg_ws_carve(nullptr, rows, n_types, n, rg_slices(slices)).bytes;
}

int rg_begin(RgWs& w, unsigned& grid, void* ws, size_t ws_bytes, const int32_t* types, const int32_t* targets, int rows,
             const int32_t* type_rowptr, int n_types, int num_products, int n, int S, int TM, int32_t* rank_out,
             int32_t* bad_count, hipStream_t st) {
    w = rg_ws_carve(ws, rows, n_types, n, S);
    if (ws_bytes < w.bytes) return PC_EWORKSPACE;
    grid = rg_item_grid(rows, n_types, S, TM);
    return rg_plan_launch(w.plan, types, targets, rows, type_rowptr, n_types, num_products, S, TM, rank_out, bad_count, st);
}
