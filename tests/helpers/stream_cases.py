"""Cases, code paths and fp64 references for the streaming kernels between the matrix kernels: csrc/bn.hip, the soft-max /
LayerNorm part of csrc/attention.hip and csrc/elementwise.hip.  CPU only: the case tables are plain tuples, path_of()
restates the dispatch conditions of the host functions (file:line next to each), the references are explicit float64
formulas (no F.batch_norm, no F.layer_norm).  tests/test_stream_cases_cover.py checks the tables against PATHS,
tests/test_gpu_stream_kernels.py runs them.

Longest chains of sequential fp32 additions (n_seq of the reduction bars, (n_seq + 8) * 2^-24 of the sum of |terms|; the
merges of the partials are fp64 and, with the roundings of the terms themselves and of the stored result, are the 8):
  bn_stats / bn_stats_thin      64  rows of a Welford group                     bn.hip:14 (STAT_ROWS), :26 / :54
  bn_bwd_reduce_kernel          64  rows of a chunk                             bn.hip:202 (BWD_ROWS), :223-232, :238
  bn_bwd_reduce2_kernel         chain(rows_per_block, rl), rl = 256 / (C / 4)   bn.hip:529, :554-573, :578
  layernorm_param_partial       64  rows of a chunk                             attention.hip:322 (LN_ROWS), :333
  colsum_partial_kernel         chain(chunk_rows, rl), rl = 256 / min(C, 256)   elementwise.hip:133-136, :151, :155
chain(n, rl): a thread adds its ceil(n / rl) rows, then row lane 0 adds the other rl - 1 lanes' sums from LDS one after the
other - ceil(n / rl) + rl - 1 additions in sequence, of which at most n have a non-zero term (64 for a 64-row chunk).
"""
import math

import torch

U = 2.0 ** -24                 # unit round-off of fp32
FLOOR = 2.0 ** -23             # floor of the measured bars: one fp32 rounding where the fp32 CPU formula happens to be exact

# ---- constants of the host functions, restated ------------------------------------------------------------------------------
STAT_ROWS = 64                 # bn.hip:14
BWD_ROWS = 64                  # bn.hip:202
FIN_STRIDE = 2048              # bn.hip:115 (bn_finalize_kernel), :257 (bn_bwd_finalize_kernel): 8 loads x 256 threads per trip
GRID_CAP = 4096                # bn.hip:359-364, elementwise.hip:10-15 (stream_grid): at most 4096 workgroups of 256 threads
BWD2_MAX_BLOCKS = 1024         # bn.hip:519
ACC_PER_CU_FWD, ACC_PER_CU_BWD = 8, 6      # bn.hip:603-608 (acc_grid): <= 256 * per_cu workgroups, >= 4 float4 per thread
SW_MAX = 64 * 8                # attention.hip:84, :163 (L <= 64 * SW_NPT: one wave per row)
SM_MAX = 256 * 32              # attention.hip:12, :159 (L <= 256 * SM_NPT)
LN_MAX = 64 * 8                # attention.hip:247, :359
LN_ROWS = 64                   # attention.hip:322
CS_ROWS = 64                   # elementwise.hip:133


def ceil_div(a, b):
    return -(-a // b)


def stream_grid(items):        # bn.hip:359, elementwise.hip:10
    return max(1, min(GRID_CAP, ceil_div(items, 256)))


def stream_trips(items):
    """trips of the busiest thread of a grid-stride loop over `items` work items"""
    return ceil_div(items, stream_grid(items) * 256)


def bn_acc_ok(C):              # ops.py:1210
    return C % 4 == 0 and C <= 1024


def bwd2_blocks(rows):         # bn.hip:587-592 -> (blocks, rows per block)
    rpb = max(64, ceil_div(rows, BWD2_MAX_BLOCKS))
    return ceil_div(rows, rpb), rpb


def acc_grid(n4, per_cu):      # bn.hip:603-608
    return max(1, min(256 * per_cu, ceil_div(n4, 256 * 4)))


def chain(n, rl):
    """longest chain of sequential fp32 additions of a chunk of n rows summed by rl row lanes and merged by lane 0"""
    return min(n, ceil_div(n, rl) + rl - 1)


def colsum_chunk_rows(rows):   # elementwise.hip:134-137
    return max(CS_ROWS, ceil_div(rows, 8192))


def pool_out(n):               # elementwise.hip:460
    return (n + 2 - 3) // 2 + 1


# ---- case tables ------------------------------------------------------------------------------------------------------------
FORMS = ("y", "beta", "none")  # (relu, y given) / (relu, y rebuilt from beta) / (no relu)
LONG_FIN = 131072 + 64 + 5     # > 2048 chunks of 64 rows: second trip of the finalize loops, and a tail chunk of 5 rows
LONG_APPLY = 360000            # x 3 channels > 4096 * 256: second trip of the scalar apply loops

# classic backward: (entry, rows, C, form, dres, accumulate).  entry "ops": ops.bn_bwd must send this C to buctd_bn_bwd
BN_BWD = ([("ops", 105, 3, f, d, a) for f in FORMS for d in (0, 1) for a in (0, 1)] +
          [("ops", LONG_FIN, 3, f, d, 1 - d) for f in FORMS for d in (0, 1)] +
          [("ops", LONG_APPLY, 3, f, 0, 0) for f in FORMS] +
          [("ops", 130, 2048, f, 1, a) for f, a in zip(FORMS, (0, 1, 0))] +
          [("direct", 4100, C, f, 1, a) for C in (48, 1024) for f, a in zip(FORMS, (1, 0, 1))])
BN_BWD_PARTIALS = [(4100, 48, f, 1, a) for f, a in zip(FORMS, (0, 1, 0))]

# statistics: (rows, C, explicit per-group counts)
BN_STATS = ([(r, C, 0) for C in (1, 2, 3, 4, 5, 48, 300) for r in (1, 63, 64, 65, 64 * 4 * 3 + 17)] +
            [(131072 + 64 * 9 + 3, C, k) for C in (3, 8) for k in (0, 1)] + [(64 * 4 * 3 + 17, 5, 1)])
# apply: (rows, C, residual, relu)
BN_APPLY = ([(r, C, res, relu) for (r, C) in ((65, 3), (130, 48), (7, 5)) for res in (0, 1) for relu in (0, 1)] +
            [(87500, 48, 1, 1), (LONG_APPLY, 3, 1, 1)])
BN_FOLD = [1, 256, 257]

# accumulator path: backward (N, H, W, C, form); the group launch: members (N, H, W, C, form, residual, acc_ready)
BN_ACC_BWD = [(12, 96, 72, 48, f) for f in FORMS]
BN_ACC_GROUP = [((2, 24, 18, 48, "y", 1, 0), (2, 12, 9, 96, "beta", 0, 1), (2, 6, 5, 192, "none", 0, 0))]

# soft-max: (rows, L, logit spread): 3.0 = normal logits of sigma 3; a larger spread S = the scaled logits cover [-1.5 S, 0]
# evenly, so that with S = 80 the lowest part of the row is below exp's fp32 underflow (e^-104 = 0, denormal from e^-87.3)
SOFTMAX_L = (1, 63, 64, 65, 512, 513, 8191, 8192)
SOFTMAX = [(r, L, 3.0) for L in SOFTMAX_L for r in (1, 5, 8)] + [(1, 513, 80.0), (5, 512, 80.0)]
SOFTMAX_SCALE = 0.37
SOFTMAX_SCALE32 = float(torch.tensor(SOFTMAX_SCALE, dtype=torch.float32))      # what the kernels receive
SOFTMAX_DROP = [(5, 64, 3.0), (5, 512, 3.0), (5, 513, 3.0), (1, 8192, 3.0)]

# LayerNorm: (rows, C)
LAYERNORM = [(r, C) for C in (1, 63, 64, 65, 112, 300, 512) for r in (1, 3, 64, 65, 130)]

# element-wise: element counts (vector body, scalar tail, both, more than one grid-stride trip)
EW_ALL = 1 << 20               # up to here every element-wise kernel runs; beyond, one per kernel source loop
EW_N = (1, 3, 4, 5, 1023, 1024, 1027, 4 * GRID_CAP * 256 + 4 * 256 + 3)
ADD_N = [(n, k) for n in (3, 4, 1027) for k in (2, 3, 4)] + [(4 * GRID_CAP * 256 + 7, 4)]
COLSUM = [(rows, C, a) for (rows, C) in ((1000, 48), (70, 300), (1, 7), (130, 64), (64 * 8192 + 64 * 3 + 1, 3)) for a in (0, 1)]
# fuse_sum: (N, H, W, C, shifts, relu); fuse_sum_bwd: (N, H, W, C, shift, y given)
FUSE_SUM = [(2, 8, 16, 8, (0,), 1), (2, 8, 16, 8, (0, 1), 0), (1, 8, 16, 12, (1, 0, 2, 3), 1), (2, 8, 8, 4, (0, 3), 0),
            (1, 16, 8, 4, (3, 2, 1, 0), 1)]
FUSE_SUM_BWD = [(2, 8, 16, 8, s, y) for s in (0, 1, 3) for y in (0, 1)]
COPY_CHANNELS = [(37, 7, 2, 11, 5, 3), (300, 48, 0, 48, 0, 48), (5, 4, 3, 9, 8, 1)]      # rows, Cs, cs0, Cd, cd0, Cc
ADD_BCAST = [(3, 35), (1, 1), (4, 1024)]                                                  # batch, n
# transposes: (N, Ctot, c0, Cc, H, W)
TRANSPOSE = [(2, 40, 3, 33, 5, 13), (1, 3, 0, 3, 9, 8), (2, 64, 0, 64, 8, 8), (3, 37, 36, 1, 1, 1), (1, 70, 5, 65, 13, 10)]
# bilinear resize: (N, Ctot, c0, Cc, H, W, Ho, Wo)
RESIZE = [(2, 5, 1, 3, 7, 5, 14, 10), (1, 3, 0, 3, 7, 5, 17, 11), (2, 4, 0, 4, 16, 12, 5, 7), (1, 2, 1, 1, 1, 1, 3, 4),
          (1, 3, 0, 3, 6, 4, 6, 4), (2, 3, 0, 3, 9, 7, 3, 1)]
# max-pool 3x3 stride 2 pad 1: (N, H, W, C, ties)
MAXPOOL = [(2, H, W, 3, t) for (H, W) in ((1, 1), (1, 2), (2, 1), (2, 2), (5, 4), (7, 7), (8, 6)) for t in (0, 1)]


# ---- paths ------------------------------------------------------------------------------------------------------------------
def _fin(n):                   # bn.hip:115, :257
    return "finalize:one-trip" if n <= FIN_STRIDE else "finalize:second-trip"


def _apply(rows, C):           # bn.hip:408-413 (bn_apply), :460-465 / :491-496 (bn_bwd_apply): the template and the trips
    vec = C % 4 == 0
    trips = stream_trips(rows * C // 4 if vec else rows * C)
    return "apply:%s%s" % ("vec" if vec else "scalar", "" if trips == 1 else "-second-trip")


def _reduce2(rows, C):         # bn.hip:554-573: does any thread run the unrolled-by-4 body, does any run the remainder
    nb, rpb = bwd2_blocks(rows)
    rl = 256 // (C // 4)
    unrolled = remainder = False
    for b in range(nb):
        r1 = min(rows, (b + 1) * rpb)
        for tr in range(rl):
            r = b * rpb + tr
            while r + 3 * rl < r1:
                unrolled, r = True, r + 4 * rl
            remainder |= r < r1
    return "reduce2:" + "+".join(n for n, on in (("unrolled", unrolled), ("remainder", remainder)) if on)


def _ew(n):                    # elementwise.hip:20-34: float4 body for n >> 2 items, scalar tail for the n % 4 last
    body, tail = n >> 2, n % 4
    names = {"ew:body" if body else "ew:no-body", "ew:tail-%d" % tail if tail else "ew:no-tail"}
    if body and stream_trips(ceil_div(n, 4)) > 1:
        names.add("ew:second-trip")
    return names


def path_of(kernel, case):
    """-> the set of path names `case` takes through `kernel` (every name is listed in PATHS[kernel])"""
    if kernel == "bn_bwd":
        entry, rows, C, form, dres, acc = case
        names = {"form:" + form, "dres:%d" % dres, "accumulate:%d" % acc}
        if entry == "ops":                                   # ops.py:1238: the accumulator path takes every C it can
            assert not bn_acc_ok(C), "ops.bn_bwd sends this C to the accumulator path"
            names.add("entry:ops-classic")
        else:
            names.add("entry:direct")
        if C % 4 == 0 and C // 4 <= 256:                     # bn.hip:444
            names.add(_reduce2(rows, C))
            nparts = bwd2_blocks(rows)[0]
        else:
            names.add("reduce:classic" if C <= 256 else "reduce:classic-cb-sweep")       # bn.hip:217
            nparts = ceil_div(rows, BWD_ROWS)
            if rows % BWD_ROWS:
                names.add("reduce:tail-chunk")
        names |= {_fin(nparts), _apply(rows, C)}
        return names
    if kernel == "bn_bwd_from_partials":
        rows, C, form, dres, acc = case
        return {"form:" + form, _fin(bwd2_blocks(rows)[0]), _apply(rows, C)}
    if kernel == "bn_stats":
        rows, C, counts = case
        ng = ceil_div(rows, STAT_ROWS)
        names = {_fin(ng), "counts:explicit" if counts else "counts:implicit"}
        if 1 <= C <= 4:                                      # bn.hip:380-383
            names.add("stats:thin-C%d" % C)
            if rows % STAT_ROWS:
                names.add("thin:last-group-short")           # bn.hip:48, :51
            if ng % 4:
                names.add("thin:idle-waves")                 # bn.hip:46
        else:
            names.add("stats:general" if C <= 256 else "stats:general-c-loop")           # bn.hip:24
            if rows % STAT_ROWS:
                names.add("general:last-group-short")
        return names
    if kernel == "bn_apply":
        rows, C, res, relu = case
        return {_apply(rows, C), "res:%d" % res, "relu:%d" % relu}
    if kernel == "bn_fold":                                  # bn.hip:350, :505
        return {"fold:blocks-%d%s" % (ceil_div(case, 256), "" if case % 256 == 0 else "-ragged")}
    if kernel == "bn_acc_bwd":
        N, H, W, C, form = case
        assert bn_acc_ok(C)
        n4 = N * H * W * C // 4
        step = acc_grid(n4, ACC_PER_CU_BWD) * 256            # bn.hip:979: two elements per trip
        return {"form:" + form, "acc-bwd:trips-%d" % min(2, ceil_div(n4, 2 * step)),
                "acc-bwd:reduce2-rpb-%s" % ("64" if bwd2_blocks(N * H * W)[1] == 64 else "long")}
    if kernel == "bn_acc_group":
        names = {"group:members-%d" % len(case)}
        for (N, H, W, C, form, res, ready) in case:
            assert bn_acc_ok(C)
            names |= {"form:" + form, "acc_ready:%d" % ready, "res:%d" % res}
        return names
    if kernel == "softmax":
        rows, L, spread = case
        assert L <= SM_MAX
        if L <= SW_MAX:                                      # attention.hip:163, :178
            names = {"softmax:wave", "wave:full-lanes" if L % 64 == 0 else "wave:ragged-lanes"}
            if rows % 4:
                names.add("wave:idle-waves")                 # attention.hip:92, :131
            if L == SW_MAX:
                names.add("softmax:wave-limit")
        else:
            names = {"softmax:block", "block:full" if L == SM_MAX else "block:ragged"}
            if L == SW_MAX + 1:
                names.add("softmax:block-first")
        if L == 1:
            names.add("softmax:single-column")
        if 1.5 * spread > 104.0:                             # scaled logits span [-1.5 * spread, 0]: exp(-104) is 0 in fp32
            names.add("softmax:underflow")
        return names
    if kernel == "layernorm":
        rows, C = case
        assert C <= LN_MAX
        names = {"ln:C<64" if C < 64 else "ln:C=64" if C == 64 else "ln:C=limit" if C == LN_MAX else "ln:C>64"}
        if rows % 4:
            names.add("ln:idle-waves")                       # attention.hip:257, :297
        if C > 256:
            names.add("ln-param:c-loop")                     # attention.hip:331
        names.add("ln-param:tail-chunk" if rows % LN_ROWS else "ln-param:whole-chunks")
        names.add("ln-param:chunks-%s" % ("1" if rows <= LN_ROWS else "n"))
        return names
    if kernel == "ew":
        return _ew(case)
    if kernel == "add_n":
        n, k = case
        return _ew(n) | {"add_n:terms-%d" % k}
    if kernel == "colsum":
        rows, C, acc = case
        cr = colsum_chunk_rows(rows)
        names = {"accumulate:%d" % acc, "colsum:long-chunks" if cr > CS_ROWS else "colsum:64-row-chunks"}   # elementwise.hip:136
        names.add("colsum:cb-sweep" if C > 256 else "colsum:C-divides-256" if 256 % C == 0 else "colsum:C-ragged")  # :141-147
        if rows % cr:
            names.add("colsum:tail-chunk")
        return names
    if kernel == "fuse_sum":
        N, H, W, C, shifts, relu = case
        return {"fuse:terms-%d" % len(shifts), "relu:%d" % relu} | {"fuse:shift-%d" % s for s in shifts}
    if kernel == "fuse_sum_bwd":
        N, H, W, C, s, y = case
        return {"fuse-bwd:shift-%d" % s, "fuse-bwd:y" if y else "fuse-bwd:y-null"}
    if kernel == "copy_channels":
        rows, Cs, cs0, Cd, cd0, Cc = case
        return {"copy:slice" if (Cc < Cs or Cc < Cd) else "copy:whole"}
    if kernel == "add_bcast":
        return {"bcast:batch-%s" % ("1" if case[0] == 1 else "n")}
    if kernel == "transpose":
        N, Ct, c0, Cc, H, W = case
        return {"tr:C%%32=%s" % ("0" if Cc % 32 == 0 else "r"), "tr:HW%%64=%s" % ("0" if (H * W) % 64 == 0 else "r"),
                "tr:slice" if Cc < Ct else "tr:whole"}
    if kernel == "resize":
        N, Ct, c0, Cc, H, W, Ho, Wo = case
        names = {"resize:slice" if Cc < Ct else "resize:whole"}
        for a, b in ((H, Ho), (W, Wo)):
            names.add("resize:same" if a == b else ("resize:up" if b > a else "resize:down") + ("" if max(a, b) % min(a, b) == 0 else "-ragged"))
        return names
    if kernel == "maxpool":
        N, H, W, C, ties = case
        return {"pool:H-%s" % ("1" if H == 1 else "2" if H == 2 else "odd" if H % 2 else "even"),
                "pool:W-%s" % ("1" if W == 1 else "2" if W == 2 else "odd" if W % 2 else "even"), "pool:ties-%d" % ties}
    raise KeyError(kernel)


TABLES = {
    "bn_bwd": BN_BWD, "bn_bwd_from_partials": BN_BWD_PARTIALS, "bn_stats": BN_STATS, "bn_apply": BN_APPLY, "bn_fold": BN_FOLD,
    "bn_acc_bwd": BN_ACC_BWD, "bn_acc_group": BN_ACC_GROUP, "softmax": SOFTMAX, "layernorm": LAYERNORM, "ew": list(EW_N),
    "add_n": ADD_N, "colsum": COLSUM, "fuse_sum": FUSE_SUM, "fuse_sum_bwd": FUSE_SUM_BWD, "copy_channels": COPY_CHANNELS,
    "add_bcast": ADD_BCAST, "transpose": TRANSPOSE, "resize": RESIZE, "maxpool": MAXPOOL,
}

# every path a kernel has; each must be taken by at least one case of its table
PATHS = {
    "bn_bwd": ["entry:ops-classic", "entry:direct", "form:y", "form:beta", "form:none", "dres:0", "dres:1", "accumulate:0",
               "accumulate:1", "reduce:classic", "reduce:classic-cb-sweep", "reduce:tail-chunk", "reduce2:unrolled",
               "reduce2:unrolled+remainder", "finalize:one-trip", "finalize:second-trip", "apply:scalar",
               "apply:scalar-second-trip", "apply:vec", "apply:vec-second-trip"],
    "bn_bwd_from_partials": ["form:y", "form:beta", "form:none", "finalize:one-trip", "apply:vec"],
    "bn_stats": ["stats:thin-C1", "stats:thin-C2", "stats:thin-C3", "stats:thin-C4", "thin:last-group-short", "thin:idle-waves",
                 "stats:general", "stats:general-c-loop", "general:last-group-short", "finalize:one-trip",
                 "finalize:second-trip", "counts:implicit", "counts:explicit"],
    "bn_apply": ["apply:vec", "apply:vec-second-trip", "apply:scalar", "apply:scalar-second-trip", "res:0", "res:1", "relu:0",
                 "relu:1"],
    "bn_fold": ["fold:blocks-1-ragged", "fold:blocks-1", "fold:blocks-2-ragged"],
    "bn_acc_bwd": ["form:y", "form:beta", "form:none", "acc-bwd:trips-2", "acc-bwd:reduce2-rpb-long"],
    "bn_acc_group": ["group:members-3", "form:y", "form:beta", "form:none", "acc_ready:0", "acc_ready:1", "res:0", "res:1"],
    "softmax": ["softmax:wave", "softmax:block", "wave:full-lanes", "wave:ragged-lanes", "wave:idle-waves", "softmax:wave-limit",
                "softmax:block-first", "block:full", "block:ragged", "softmax:single-column", "softmax:underflow"],
    "layernorm": ["ln:C<64", "ln:C=64", "ln:C>64", "ln:C=limit", "ln:idle-waves", "ln-param:c-loop", "ln-param:tail-chunk",
                  "ln-param:whole-chunks", "ln-param:chunks-1", "ln-param:chunks-n"],
    "ew": ["ew:body", "ew:no-body", "ew:no-tail", "ew:tail-1", "ew:tail-3", "ew:second-trip"],
    "add_n": ["add_n:terms-2", "add_n:terms-3", "add_n:terms-4", "ew:body", "ew:no-body", "ew:tail-3", "ew:no-tail",
              "ew:second-trip"],
    "colsum": ["accumulate:0", "accumulate:1", "colsum:64-row-chunks", "colsum:long-chunks", "colsum:C-divides-256",
               "colsum:C-ragged", "colsum:cb-sweep", "colsum:tail-chunk"],
    "fuse_sum": ["fuse:terms-1", "fuse:terms-2", "fuse:terms-4", "fuse:shift-0", "fuse:shift-1", "fuse:shift-2", "fuse:shift-3",
                 "relu:0", "relu:1"],
    "fuse_sum_bwd": ["fuse-bwd:shift-0", "fuse-bwd:shift-1", "fuse-bwd:shift-3", "fuse-bwd:y", "fuse-bwd:y-null"],
    "copy_channels": ["copy:slice", "copy:whole"],
    "add_bcast": ["bcast:batch-1", "bcast:batch-n"],
    "transpose": ["tr:C%32=0", "tr:C%32=r", "tr:HW%64=0", "tr:HW%64=r", "tr:slice", "tr:whole"],
    "resize": ["resize:slice", "resize:whole", "resize:same", "resize:up", "resize:up-ragged", "resize:down", "resize:down-ragged"],
    "maxpool": ["pool:H-1", "pool:H-2", "pool:H-odd", "pool:H-even", "pool:W-1", "pool:W-2", "pool:W-odd", "pool:W-even",
                "pool:ties-0", "pool:ties-1"],
}

# the cases that exist to reach a second loop trip, and the trip they must reach: (kernel, case filter, path name)
SECOND_TRIPS = [
    ("bn_bwd", lambda c: c[1] == LONG_FIN, "finalize:second-trip"),
    ("bn_bwd", lambda c: c[1] == LONG_APPLY, "apply:scalar-second-trip"),
    ("bn_stats", lambda c: c[0] > 131072, "finalize:second-trip"),
    ("bn_apply", lambda c: c[0] == 87500, "apply:vec-second-trip"),
    ("bn_apply", lambda c: c[0] == LONG_APPLY, "apply:scalar-second-trip"),
    ("bn_acc_bwd", lambda c: True, "acc-bwd:trips-2"),
    ("colsum", lambda c: c[0] > 64 * 8192, "colsum:long-chunks"),
    ("ew", lambda c: c > 4 * GRID_CAP * 256, "ew:second-trip"),
    ("add_n", lambda c: c[0] > 4 * GRID_CAP * 256, "ew:second-trip"),
]


def case_bytes(kernel, case):
    """bytes of all operands and outputs (fp32 / int32) and of the references kept for the comparison (fp64, or fp32 where the
    bar is bit-exact) of one case; temporaries of the reference formulas are not counted"""
    f, d = 4, 8
    if kernel in ("bn_bwd", "bn_bwd_from_partials"):
        rows, C = (case[1], case[2]) if kernel == "bn_bwd" else (case[0], case[1])
        return rows * C * (5 * f + d + f + f) + ceil_div(rows, 64) * 2 * C * f    # dy y z dz dres | dz fp64, dres, dz fp32
    if kernel == "bn_stats":
        return case[0] * case[1] * (f + 2 * d) + ceil_div(case[0], 64) * case[1] * 3 * f
    if kernel == "bn_apply":
        return case[0] * case[1] * (3 * f + 3 * d)
    if kernel == "bn_fold":
        return case * 6 * (f + d)
    if kernel == "bn_acc_bwd":
        return math.prod(case[:4]) * (5 * f + d + f + f)
    if kernel == "bn_acc_group":
        return sum(math.prod(m[:4]) * (7 * f + 5 * d) for m in case)
    if kernel == "softmax":
        return case[0] * case[1] * (5 * f + 4 * d)
    if kernel == "layernorm":
        return case[0] * case[1] * (6 * f + 5 * d)
    if kernel == "ew":                            # a, b, y | seven outputs (four at the long size) | one fp32 reference at a time
        return case * f * (3 + (7 if case <= EW_ALL else 4) + 1)
    if kernel == "add_n":
        return case[0] * (case[1] + 2) * f
    if kernel == "colsum":
        return case[0] * case[1] * (f + 2 * d)
    if kernel in ("fuse_sum", "fuse_sum_bwd"):
        return math.prod(case[:4]) * 6 * (f + d)
    if kernel == "copy_channels":
        return case[0] * (case[1] + 2 * case[3]) * f
    if kernel == "add_bcast":
        return case[0] * case[1] * 3 * f
    if kernel == "transpose":
        return case[0] * case[1] * case[4] * case[5] * 4 * f
    if kernel == "resize":
        return (case[0] * case[1] * case[4] * case[5] + case[0] * case[3] * case[6] * case[7] * 3) * (f + d)
    if kernel == "maxpool":
        return math.prod(case[:4]) * 6 * (f + d)
    raise KeyError(kernel)


# ---- operands ---------------------------------------------------------------------------------------------------------------
def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (hash(k) if not isinstance(k, int) else k)) & 0x7FFFFFFF
    return torch.Generator().manual_seed(seed)


def _key(case):
    out = []
    for k in case:
        if isinstance(k, (tuple, list)):
            out += _key(k)
        elif isinstance(k, str):
            out.append(sum(ord(ch) * (i + 1) for i, ch in enumerate(k)))
        else:
            out.append(int(k * 16) if isinstance(k, float) else int(k))
    return out


def case_gen(kernel, case):
    return gen(*_key((kernel,) + (tuple(case) if isinstance(case, (tuple, list)) else (case,))))


def channel_data(g, rows, C):
    """[rows, C] fp32 with a per-channel mean of a few sigma: sigma in [0.5, 2), mean in +-3 sigma"""
    sig = 0.5 + 1.5 * torch.rand(C, generator=g)
    mu = (torch.rand(C, generator=g) * 6 - 3) * sig
    return torch.randn(rows, C, generator=g) * sig + mu


def bn_params(g, C):
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    gamma = torch.where(gamma.abs() < 0.2, torch.full_like(gamma, 0.5), gamma)
    return gamma, 0.2 * torch.randn(C, generator=g)


# ---- fp64 references --------------------------------------------------------------------------------------------------------
EPS = 1e-5


def bn_stats_ref(z):
    """z [rows, C] (any float type) -> mean, biased var, sum |z| / rows   (fp64)"""
    z = z.double()
    rows = z.shape[0]
    mean = z.sum(0) / rows
    var = ((z - mean) ** 2).sum(0) / rows
    return mean, var, z.abs().sum(0) / rows


def bn_apply_ref(z, mean, invstd, gamma, beta, res=None, relu=False, dtype=torch.float64):
    """the expression of bn_apply_kernel in `dtype`: (z - mean) * (invstd * gamma) + beta (+ res), relu"""
    z, mean, invstd, gamma, beta = (t.to(dtype) for t in (z, mean, invstd, gamma, beta))
    y = (z - mean) * (invstd * gamma) + beta
    if res is not None:
        y = y + res.to(dtype)
    return torch.relu(y) if relu else y


def bn_bwd_ref(dy, z, mean, invstd, gamma, mask, dtype=torch.float64):
    """-> dz, dres (= masked dy), s1 (dbeta), s2 (dgamma), sum |g|, sum |g zhat|; mask: bool [rows, C] or None"""
    dy, z, mean, invstd, gamma = (t.to(dtype) for t in (dy, z, mean, invstd, gamma))
    rows = z.shape[0]
    g = dy if mask is None else torch.where(mask, dy, torch.zeros_like(dy))
    zh = (z - mean) * invstd
    t2 = g * zh
    s1, s2 = g.sum(0), t2.sum(0)
    dz = gamma * invstd * (g - s1 / rows - zh * s2 / rows)
    return dz, g, s1, s2, g.abs().sum(0), t2.abs().sum(0)


def bn_bwd_operands(kernel, case, rows, C, form):
    """z, dy, mean, invstd (fp32, from the fp64 statistics of z), gamma, beta, y (or None), mask (or None): no ReLU
    pre-activation within 1e-4 of zero"""
    g = case_gen(kernel, case)
    z = channel_data(g, rows, C)
    dy = torch.randn(rows, C, generator=g)
    gamma, beta = bn_params(g, C)
    res = torch.randn(rows, C, generator=g) if form == "y" else None
    for _ in range(4):
        mean, var, _ = bn_stats_ref(z)
        mean, invstd = mean.float(), (1.0 / torch.sqrt(var + EPS)).float()
        if form == "none":
            return z, dy, mean, invstd, gamma, beta, None, None
        pre = bn_apply_ref(z, mean, invstd, gamma, beta, res)
        bad = pre.abs() < 1e-4
        if not bool(bad.any()):
            y = torch.relu(pre).float() if form == "y" else None
            return z, dy, mean, invstd, gamma, beta, y, pre > 0
        if form == "y":
            res = torch.where(bad, res + 0.01, res)          # the residual moves the pre-activation, not the statistics
        else:
            z = torch.where(bad, z + 0.01, z)                # the statistics are taken again from the pushed z
    raise AssertionError("could not clear the ReLU ties")


def softmax_ref(s, scale, dp=None):
    """-> p (and ds for the gradient dp of p): fp64"""
    x = s.double() * scale
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)
    if dp is None:
        return p
    dp = dp.double()
    return p, scale * p * (dp - (dp * p).sum(-1, keepdim=True))


def layernorm_ref(x, gamma, beta, eps, dtype=torch.float64):
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / C
    var = ((x - mean) ** 2).sum(-1, keepdim=True) / C
    invstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * invstd * gamma + beta, mean.squeeze(-1), invstd.squeeze(-1)


def layernorm_bwd_ref(dy, x, mean, invstd, gamma, dtype=torch.float64):
    """-> dx, dgamma, dbeta, sum |dy xhat|, sum |dy| (per column)"""
    dy, x, mean, invstd, gamma = (t.to(dtype) for t in (dy, x, mean, invstd, gamma))
    C = x.shape[-1]
    xh = (x - mean[:, None]) * invstd[:, None]
    gy = dy * gamma
    s1 = gy.sum(-1, keepdim=True) / C
    s2 = (gy * xh).sum(-1, keepdim=True) / C
    dx = invstd[:, None] * (gy - s1 - xh * s2)
    t = dy * xh
    return dx, t.sum(0), dy.sum(0), t.abs().sum(0), dy.abs().sum(0)


def nearest_up(t, s):
    """[N, h, w, C] -> [N, h << s, w << s, C]: out[h][w] = t[h >> s][w >> s]"""
    f = 1 << s
    return t.repeat_interleave(f, 1).repeat_interleave(f, 2)


def fuse_sum_ref(terms, shifts, relu, dtype=torch.float64):
    out = None
    for t, s in zip(terms, shifts):                           # left to right, as the kernel adds them
        u = nearest_up(t.to(dtype), s)
        out = u if out is None else out + u
    out = torch.zeros_like(out) + out                         # (the kernel starts from zero: 0 + t0 is exact)
    return torch.relu(out) if relu else out


def fuse_sum_bwd_ref(dy, y, s, dtype=torch.float64):
    """-> g, sum of |terms|: the f x f window sums, rows outer, columns inner"""
    d = dy.to(dtype)
    if y is not None:
        d = torch.where(y > 0, d, torch.zeros_like(d))
    N, H, W, C = d.shape
    f = 1 << s
    d = d.view(N, H // f, f, W // f, f, C)
    acc = torch.zeros(N, H // f, W // f, C, dtype=dtype)
    mag = torch.zeros_like(acc)
    for dh in range(f):
        for dw in range(f):
            acc = acc + d[:, :, dh, :, dw, :]
            mag = mag + d[:, :, dh, :, dw, :].abs()
    return acc, mag


def resize_ref(x, c0, cc, Ho, Wo, dtype=torch.float64):
    """bilinear, align_corners=False, no antialias: src = max((dst + 0.5) * in / out - 0.5, 0).  x NCHW -> NHWC, and the sum
    of |weight * value| per output.  In `dtype` from the scale on (the fp32 evaluation follows the kernel's own steps)."""
    N, Ct, H, W = x.shape
    xs = x[:, c0:c0 + cc].to(dtype)

    def axis(n_in, n_out):
        sc = torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)
        f = (torch.arange(n_out, dtype=dtype) + 0.5) * sc - 0.5
        f = torch.clamp(f, min=0)
        i0 = f.floor().long()
        i1 = i0 + (i0 < n_in - 1).long()
        l1 = f - i0.to(dtype)
        return i0, i1, 1 - l1, l1
    y0, y1, hy, ly = axis(H, Ho)
    x0, x1, hx, lx = axis(W, Wo)

    def at(yy, xx):
        return xs[:, :, yy][:, :, :, xx]
    hx, lx = hx[None, None, None, :], lx[None, None, None, :]
    hy, ly = hy[None, None, :, None], ly[None, None, :, None]
    out = hy * (hx * at(y0, x0) + lx * at(y0, x1)) + ly * (hx * at(y1, x0) + lx * at(y1, x1))
    mag = hy * (hx * at(y0, x0).abs() + lx * at(y0, x1).abs()) + ly * (hx * at(y1, x0).abs() + lx * at(y1, x1).abs())
    return out.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()


def maxpool_ref(x):
    """3x3 stride 2 pad 1 on NHWC, the first maximum in (row, column) order wins -> y, idx (hi * W + wi), exact"""
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    y = torch.full((N, Ho, Wo, C), float("-inf"), dtype=x.dtype)
    idx = torch.full((N, Ho, Wo, C), -1, dtype=torch.int32)
    for ho in range(Ho):
        for wo in range(Wo):
            for r in range(3):
                for s in range(3):
                    hi, wi = 2 * ho - 1 + r, 2 * wo - 1 + s
                    if 0 <= hi < H and 0 <= wi < W:
                        v = x[:, hi, wi, :]
                        better = (idx[:, ho, wo, :] < 0) | (v > y[:, ho, wo, :])
                        y[:, ho, wo, :] = torch.where(better, v, y[:, ho, wo, :])
                        idx[:, ho, wo, :] = torch.where(better, torch.full_like(idx[:, ho, wo, :], hi * W + wi), idx[:, ho, wo, :])
    return y, idx


def maxpool_bwd_ref(dy, idx, shape):
    """scatter of dy to its argmax, fp64 (windows overlap: up to four outputs may name one input)"""
    N, H, W, C = shape
    dx = torch.zeros(N, H * W, C, dtype=torch.float64)
    n_hit = torch.zeros(N, H * W, C, dtype=torch.int64)
    flat = idx.reshape(N, -1, C).long()
    dx.scatter_add_(1, flat, dy.double().reshape(N, -1, C))
    n_hit.scatter_add_(1, flat, torch.ones_like(flat))
    return dx.view(N, H, W, C), n_hit.view(N, H, W, C)
