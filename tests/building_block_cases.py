"""Case lists, input builders and bounds of the building-block tests (test_gpu_building_blocks.py runs them on the
GPU, test_building_block_bounds_host.py checks on the CPU that the lists cover what they claim and that the bounds
cannot reject a correct kernel).  Pure torch / numpy: importable without a GPU.

The `nt_form` / `tn_form` functions restate the launchers' own dispatch conditions (launch_variant in gemm_nt.hip,
tn_full_tile / tn_plan in gemm_tn.hip) so that a case list can be checked against the form it is named after."""
import torch

# ------------------------------------------------------------------ inputs
def randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def linear_inputs(rows, in_dim, out_dim, bias=True, seed=0):
    """x [rows,in], w [out,in] * 0.1 (pre-activations O(1), as test_gpu_ops.test_linear_forward), b [out] or None"""
    x = randn(rows, in_dim, seed=100 + seed)
    w = randn(out_dim, in_dim, seed=200 + seed, scale=0.1)
    b = randn(out_dim, seed=300 + seed) if bias else None
    return x, w, b


def dx_inputs(rows, out_dim, in_dim, seed=0):
    return randn(rows, out_dim, seed=400 + seed), randn(out_dim, in_dim, seed=500 + seed, scale=0.1)


def dw_inputs(rows, out_dim, in_dim, x_rows=None, seed=0):
    """dy [rows,out], x [x_rows or rows, in]"""
    return randn(rows, out_dim, seed=600 + seed), randn(rows if x_rows is None else x_rows, in_dim, seed=700 + seed)


GATHER_TABLE_ROWS = 50      # linear_forward gather cases: x is a table of this many rows
TN_TABLE_ROWS = 300         # linear_backward_weight gather cases


def gather_idx(rows, table_rows, tile, seed=0):
    """Row indices with -1 rows (every 7th, the LAST row of every `tile`-row tile and the very last row, which closes
    the ragged final tile) and duplicates."""
    idx = torch.randint(0, table_rows, (rows,), generator=torch.Generator().manual_seed(800 + seed), dtype=torch.int32)
    if rows >= 4:
        idx[2] = idx[1] = 3
    idx[::7] = -1
    idx[tile - 1::tile] = -1
    idx[rows - 1] = -1
    return idx


def sparse_idx(rows, table_rows, seed=0, p_skip=0.1):
    """about 10 % -1 entries, the rest uniform over the table (duplicates as soon as rows > a few)"""
    g = torch.Generator().manual_seed(900 + seed)
    idx = torch.randint(0, table_rows, (rows,), generator=g, dtype=torch.int32)
    idx[torch.rand(rows, generator=g) < p_skip] = -1
    return idx


def gathered(table, idx):
    """table[idx] with a zero row for every -1"""
    tab = torch.cat([table, torch.zeros(1, table.shape[1], dtype=table.dtype, device=table.device)])
    return tab[torch.where(idx < 0, table.shape[0], idx.long())]


# ------------------------------------------------------------------ the project's fp32-grade bound
# (test_gpu_ops.test_matrix_core_products_fp32_grade_on_adversarial_operands): per element
#   |y - ref| <= 1.25 max|torch_fp32 - ref| + 4e-7 mag + 1.2e-38,    mag = |x| |w|^T + |b|
# 4e-7 mag is what an exact-fp32 fma chain is allowed; TANH_ABS is what test_linear_forward grants fast_tanh on O(1)
# pre-activations.  tanh and ReLU are 1-Lipschitz, so the bound of the pre-activation holds behind them.
MAG_COEF = 4e-7
FP32_TINY = 1.2e-38
TANH_ABS = 2e-5


def fp32_grade_tol(e32_max, mag, act=0):
    return 1.25 * e32_max + MAG_COEF * mag + FP32_TINY + (TANH_ABS if act == 1 else 0.0)


# ------------------------------------------------------------------ launch_gemm_nt: which kernel form a product takes
NT_FORMS = ("few_row", "two_wave", "four_wave", "paired_four_wave", "eight_wave_1", "eight_wave_2", "eight_wave_3plus")
NT_TILE = {"few_row": 32, "two_wave": 64}           # rows per tile (every other form: 128)


def nt_form(m, k, n):
    """launch_variant<false, NONE|TANH|RELU, no statistics>: ntm = ceil(M / 128) row tiles; ntm >= 192 <=> M >= 24449"""
    ntm = (m + 127) // 128
    if 128 < n <= 256 and ntm >= 192:
        return "paired_four_wave"
    if n > 128:
        return ("eight_wave_1", "eight_wave_2")[(n + 255) // 256 - 1] if n <= 512 else "eight_wave_3plus"
    if ntm >= 192:
        return "four_wave"
    return "few_row" if k <= 256 else "two_wave"


def nt_paired_tiles(m):
    """(row tiles, tiles of the paired numbering): whole groups of 16, the excess are padding tiles without rows"""
    ntm = (m + 127) // 128
    return ntm, (2 * ntm + 15) & ~15


# (M, K, N, act, bias, gather): act 0 none / 1 tanh / 2 relu.  Every list holds each value of the issue's table for its
# form, bias and no bias, the three activations and one gather case; K tails (K % 16, K % 32 != 0) meet every
# persistent form.  test_building_block_bounds_host.py asserts all of that.
NT_CASES = {
    # N <= 128, <= 191 row tiles, K <= 256: 32-row tiles, stage rows of 32 / 64 / 128 floats (K <= 32 / 64 / more),
    # two bursts for K in (128, 256].  K = 32|36, 64|68, 128|132 straddle the stage sizes, M = 24448 is the last few-row M.
    "few_row": [(1, 4, 1, 0, True, False), (31, 32, 3, 2, False, False), (32, 36, 33, 1, True, False),
                (33, 64, 127, 0, False, False), (33, 68, 128, 2, True, False), (32, 128, 127, 1, False, False),
                (31, 132, 33, 0, True, False), (33, 256, 128, 2, True, False), (24448, 36, 3, 0, True, False),
                (24448, 256, 128, 1, False, False), (33, 132, 127, 2, True, True)],
    # N <= 128, <= 191 row tiles, K > 256 (260: the first K past the few-row kernel): 64-row tiles, BK = 32
    "two_wave": [(1, 260, 5, 0, True, False), (63, 300, 64, 1, False, False), (64, 1028, 128, 2, True, False),
                 (65, 260, 128, 0, False, False), (200, 1028, 128, 0, True, False), (200, 300, 5, 2, False, False),
                 (65, 1028, 64, 1, True, False), (200, 260, 64, 0, True, True)],
    # N <= 128, >= 192 row tiles (M = 24449 is the first): persistent 128 x 128 tiles, BK = 16
    "four_wave": [(24449, 4, 6, 0, True, False), (24449, 20, 128, 1, False, False), (24577, 100, 6, 2, True, False),
                  (24577, 128, 128, 0, False, False), (24449, 100, 128, 0, True, False), (24577, 20, 6, 1, False, False),
                  (24577, 4, 128, 2, False, False), (24449, 100, 128, 2, True, True)],
    # 128 < N <= 256, >= 192 row tiles: two 128-wide column tiles per row tile in the paired numbering, BK = 16;
    # M = 24449: 192 row tiles = 384 tiles, no padding tile; M = 24577: 193 row tiles -> 400 tiles, 14 of them padding
    "paired_four_wave": [(24449, 36, 129, 0, True, False), (24449, 128, 132, 1, False, False),
                         (24449, 36, 255, 2, True, False), (24449, 128, 256, 0, False, False),
                         (24577, 36, 256, 1, True, False), (24577, 128, 129, 2, False, False),
                         (24577, 36, 132, 0, False, False), (24577, 128, 255, 0, True, False),
                         (24449, 36, 132, 2, True, True)],
    # 128 < N <= 256, <= 191 row tiles: 128 x 256 tiles of 8 waves, BK = 32
    "eight_wave_1": [(1, 36, 129, 0, True, False), (127, 100, 130, 1, False, False), (128, 260, 256, 2, True, False),
                     (129, 36, 256, 0, False, False), (129, 100, 129, 2, False, False), (127, 260, 130, 0, True, False),
                     (128, 36, 130, 1, True, False), (1, 260, 256, 0, False, False), (129, 100, 130, 0, True, True)],
    # 256 < N <= 512: two 256-wide column tiles per row tile (paired numbering), any M
    "eight_wave_2": [(129, 8, 257, 0, True, False), (1000, 36, 258, 1, False, False), (24449, 128, 512, 2, True, False),
                     (129, 36, 512, 0, False, False), (1000, 128, 257, 2, False, False), (24449, 8, 258, 0, False, False),
                     (1000, 8, 512, 1, True, False), (24449, 36, 257, 0, True, False), (1000, 36, 258, 2, True, True)],
    # N > 512: three and more column tiles, plain numbering
    "eight_wave_3plus": [(5, 36, 513, 0, True, False), (130, 64, 770, 1, False, False), (130, 36, 513, 2, True, False),
                         (5, 64, 770, 0, False, False), (130, 36, 770, 2, False, False), (5, 36, 770, 1, True, False),
                         (130, 64, 513, 0, True, False), (130, 36, 770, 0, True, True)],
}
# the values the issue's table lists per form: (M, K, N)
NT_LISTED = {
    "few_row": ((1, 31, 32, 33, 24448), (4, 32, 36, 64, 68, 128, 132, 256), (1, 3, 33, 127, 128)),
    "two_wave": ((1, 63, 64, 65, 200), (260, 300, 1028), (5, 64, 128)),
    "four_wave": ((24449, 24577), (4, 20, 100, 128), (6, 128)),
    "paired_four_wave": ((24449, 24577), (36, 128), (129, 132, 255, 256)),
    "eight_wave_1": ((1, 127, 128, 129), (36, 100, 260), (129, 130, 256)),
    "eight_wave_2": ((129, 1000, 24449), (8, 36, 128), (257, 258, 512)),
    "eight_wave_3plus": ((5, 130), (36, 64), (513, 770)),
}
# in_dim % 4 != 0: ops.linear_forward pads x and w with zero columns (K = 5 -> 8 few-row, K = 130 -> 132 8-wave)
NT_PADDED_K = [(33, 5, 33, 0, True, False), (129, 130, 130, 2, True, False)]
# rows= smaller than x's row count: (rows of x, rows, K, N); a ragged last tile and the scalar store path in both
NT_ROWS_ARG = [(100, 37, 36, 33), (300, 130, 36, 130)]


def nt_id(case):
    m, k, n, act, bias, gather = case
    return f"{nt_form(m, k + (-k) % 4, n)}-M{m}-K{k}-N{n}-act{act}" + ("-bias" if bias else "") + ("-gather" if gather else "")


# ------------------------------------------------------------------ linear_backward_input: (rows, out_dim, in_dim)
# dx = dy . w through the same NT forms, the contraction over out_dim (K = out_dim rounded up to 4, N = in_dim)
DX_CASES = [(1, 4, 4),            # few-row, one row, one 32 x 32 transpose tile of 4 x 4
            (1, 3, 5),            # out_dim % 4 != 0 (zero-padded) and in_dim % 4 != 0 (ldc = 5: scalar stores)
            (33, 130, 70),        # few-row, K = 130 -> 132: second burst; ragged transpose 130 x 70
            (200, 256, 128),      # the shape of test_gpu_ops.test_linear_backward_input
            (100, 300, 64),       # 2-wave (K = 300 > 256)
            (65, 1028, 128),      # 2-wave, the longest contraction
            (24449, 64, 200),     # paired 4-wave (N = 200)
            (24449, 36, 128),     # 4-wave 128 x 128, K tail
            (129, 40, 513)]       # 8-wave, three column tiles, ldc = 513


def dx_form(rows, out_dim, in_dim):
    return nt_form(rows, out_dim + (-out_dim) % 4, in_dim)


# ------------------------------------------------------------------ launch_gemm_tn
def tn_full_tile(r, no, ni):
    return r >= 8192 and no <= 256 and ni <= 256 and (no > 128 or ni > 128) and no % 64 == 0 and ni % 64 == 0


def tn_plan(r, no, ni):
    """(nsplit, rows_per_split) of gemm_tn.hip's tn_plan"""
    tiles = ((no + 127) // 128) * ((ni + 127) // 128)
    s = 256 if tn_full_tile(r, no, ni) else (512 + tiles - 1) // tiles
    s = max(1, min(s, (r + 63) // 64))
    rps = ((r + s - 1) // s + 31) // 32 * 32
    return (r + rps - 1) // rps, rps


DW_PLAIN_ROWS = (1, 31, 32, 33, 63, 64, 65, 8191)
DW_PLAIN_SHAPES = ((4, 4), (36, 132), (128, 128), (132, 260), (260, 36))
# R = 8191 is the last row count of the plain kernel for shapes the full-tile kernels take from 8192 on
DW_PLAIN_CASES = [(r, no, ni) for r in DW_PLAIN_ROWS for (no, ni) in DW_PLAIN_SHAPES] + [(8191, 256, 256), (8191, 192, 64)]
DW_PADDED_CASES = [(33, 5, 7), (65, 130, 3)]          # out_dim / in_dim % 4 != 0: ops._pad_cols
DW_FULL_SHAPES = ((256, 256), (192, 192), (192, 64), (64, 192), (256, 128), (128, 256), (256, 64), (64, 256), (192, 128),
                  (128, 192))
# 8192: the first full-tile R (128 slices of 64 rows); 8193: a ragged last slice; 19969: the non-monotone plan
# (209 slices of 96 rows -- fewer than at R = 8193 .. 16384)
DW_FULL_CASES = [(8193, no, ni) for (no, ni) in DW_FULL_SHAPES] + [(r, no, ni) for r in (8192, 19969)
                                                                  for (no, ni) in ((256, 256), (192, 64))]
DW_GATHER_CASES = [(70, 36, 132), (8193, 192, 64), (8193, 128, 256)]
DW_NO_BIAS_CASES = [(65, 36, 132), (8193, 192, 64)]

# ------------------------------------------------------------------ scatter_add_rows, integer data
# (table rows, width, source rows, mode): sources integer-valued in [-8, 8], the table starts integer-valued in [-8, 8]:
# every partial sum of any order is an integer below 2^24 in magnitude, hence exact in fp32
INT_RANGE = 8
SCATTER_INT_CASES = [(1, 1, 1, "uniform"), (1, 64, 255, "uniform"),            # every source on the one row
                     (7, 3, 257, "uniform"), (100, 64, 12288, "uniform"), (5000, 130, 257, "uniform"),
                     (100, 1, 12288, "one_row"), (7, 130, 255, "uniform"), (5000, 3, 12288, "uniform"),
                     (100, 64, 12288, "one_row"), (5000, 64, 1, "uniform")]
# pc_scatter_add_rows_small: tables that fit the 64 KB LDS copy (256 x 64 floats exactly fills it), one that does not
# (257 x 64: the launcher falls back to the global-atomic kernel); 128 source rows per workgroup up to 256 workgroups,
# 32769 rows are more than 256 x 128
SCATTER_SMALL_CASES = [(100, 64, 1, "uniform"), (100, 64, 127, "uniform"), (256, 64, 128, "uniform"),
                       (256, 64, 129, "uniform"), (100, 64, 32769, "uniform"), (256, 64, 32769, "one_row"),
                       (257, 64, 129, "uniform"), (257, 64, 32769, "uniform"), (100, 3, 129, "uniform"),
                       (7, 3, 32769, "uniform")]


def scatter_int_inputs(table_rows, width, rows, mode, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    table = torch.randint(-INT_RANGE, INT_RANGE + 1, (table_rows, width), generator=g)
    src = torch.randint(-INT_RANGE, INT_RANGE + 1, (rows, width), generator=g)
    if mode == "one_row":
        idx = torch.full((rows,), table_rows // 2, dtype=torch.int32)
    else:
        idx = torch.randint(0, table_rows, (rows,), generator=g, dtype=torch.int32)
    if rows > 2:
        idx[::11] = -1
    return table, idx, src          # int64 values; the callers convert to fp32


def scatter_int_worst_partial(table_rows, idx):
    """largest |partial sum| any order of the additions can reach on one element"""
    hits = torch.bincount(idx[idx >= 0].long(), minlength=table_rows)
    return INT_RANGE * (int(hits.max()) + 1)
