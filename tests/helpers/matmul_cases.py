"""The case table of the fp32 batched matmul tests (csrc/matmul.hip: matmul_kernel, matmul_splitk_reduce), as data.

A case is a full buctd_matmul_desc plus the element offsets of the three pointers (a_off / b_off / c_off, as ops.matmul takes
them), the bias axis (None: no bias), alpha, whether its operands are the hard ones, and the plan it must reach as
buctd_matmul_plan reports it: tile id (0 = 128x64 scalar loads, 1 = 128x48, 2 = 128x96, 3 = 128x128 vector loads; vec is
tile != 0) and the number of K splits.  The GPU test asserts the plan before it runs, so a dispatch change cannot move a case off
the kernel under test without a failure that says so.

tests/test_matmul_plan_cover.py (host only) proves that the table reaches every (layouts, tile, split state) the routing can
pick on the search grid below and every launch_mm instance of the source; tests/test_gpu_matmul_fp32.py runs every case against
fp64.  build() makes the operands and the write set of a case from the addressing formulas in the header comment of
matmul.hip alone, so the reference shares no argument handling with ops.matmul."""
import collections
import ctypes as C
import math

import torch

PLAN_FIELDS = ("tile", "BM", "BN", "WM", "MF", "vec", "nsplit", "k_per_split")
LAYOUT = {(0, 0): "rr", (0, 1): "rc", (1, 0): "cr", (1, 1): "cc"}      # A rows / cols x B rows / cols
# the base address plan() gives to the three buffers: 16-byte aligned, like every allocation of the caching allocator
BASE = 1 << 20

Case = collections.namedtuple("Case", (
    "name batch M N K a_layout b_layout lda ldb ldc stride_a stride_b stride_c Kc gsa gsbk Nc gsbn gsc "
    "a_off b_off c_off bias_axis alpha hard tile nsplit"))


def mm(name, batch, M, N, K, al, bl, tile, nsplit=1, *, lda=None, ldb=None, ldc=None, stride_a=None, stride_b=None,
       stride_c=None, Kc=None, gsa=0, gsbk=0, Nc=None, gsbn=0, gsc=0, a_off=0, b_off=0, c_off=0, bias=None, alpha=1.0, hard=0):
    """a case; what is not given is the dense packing: A [batch][M][K] (rows) or [batch][K][M] (cols), B [batch][N][K] (rows) or
    [batch][K][N] (cols), C [batch][M][N], one k-group, one n-group"""
    lda = (K if al == 0 else M) if lda is None else lda
    ldb = (K if bl == 0 else N) if ldb is None else ldb
    ldc = N if ldc is None else ldc
    stride_a = (M if al == 0 else K) * lda if stride_a is None else stride_a
    stride_b = (N if bl == 0 else K) * ldb if stride_b is None else stride_b
    stride_c = M * ldc if stride_c is None else stride_c
    return Case(name, batch, M, N, K, al, bl, lda, ldb, ldc, stride_a, stride_b, stride_c, K if Kc is None else Kc, gsa, gsbk,
                N if Nc is None else Nc, gsbn, gsc, a_off, b_off, c_off, bias, alpha, hard, tile, nsplit)


# ---- every launch form: 4 layouts x 4 tiles x {one split, exact splits, ragged last split} ------------------------------
# K = 1024 -> 4 splits of 256; K = 1040 -> 3 x 272 + 224; K = 1041 -> 3 x 272 + 225; K = 2049 -> 7 x 272 + 145 (all with one
# tile per batch entry).  Dense vector loads need K % 4 (a rows operand), M % 4 (A cols), N % 4 (B cols) and aligned pointers.
FORM_CASES = [
    # -- tile 0, 128x64 scalar loads.  Reached by odd sizes ...
    mm("odd sizes, M = 128 + 13, N = 64 + 1", 2, 141, 65, 13, 0, 0, 0, bias=0),
    mm("odd sizes, M < 16, K = 3", 3, 9, 19, 3, 0, 1, 0, alpha=-0.75),
    mm("A cols with ragged M, two row tiles", 2, 131, 21, 29, 1, 0, 0, bias=1),
    mm("A and B cols ragged, N = 64 + 3", 2, 50, 67, 72, 1, 1, 0),
    mm("B cols, N = 129: the third column tile has one column", 1, 37, 129, 16, 0, 1, 0, bias=0, alpha=0.5),
    # ... by an odd leading dimension with vector-friendly sizes ...
    mm("lda = 17", 2, 48, 48, 16, 0, 0, 0, lda=17),
    mm("ldb = 49 (B cols)", 2, 48, 48, 16, 1, 1, 0, ldb=49),
    # ... and by a pointer that is not 16-byte aligned
    mm("a_off = 2", 2, 48, 48, 16, 0, 1, 0, a_off=2),
    mm("b_off = 1", 2, 48, 96, 20, 1, 0, 0, b_off=1),
    # split-K on the scalar tile: k + j < k_end inside a split
    mm("exact splits, a_off = 1", 1, 48, 48, 1024, 0, 0, 0, 4, a_off=1),
    mm("exact splits, N = 47", 2, 16, 47, 1024, 0, 1, 0, 4),
    mm("exact splits, M = 47", 1, 47, 20, 1024, 1, 0, 0, 4),
    mm("exact splits, N = 46", 1, 48, 46, 1024, 1, 1, 0, 4, bias=0),
    mm("ragged last split, odd K", 1, 33, 17, 1041, 0, 0, 0, 4),
    mm("ragged last split, b_off = 1", 1, 20, 48, 1040, 0, 1, 0, 4, b_off=1, bias=1, alpha=0.25),
    mm("ragged last split, odd K = 2049", 1, 48, 30, 2049, 1, 0, 0, 8),
    mm("ragged last split, M = 45", 2, 45, 48, 1040, 1, 1, 0, 4),
    # -- tile 1, 128x48 vector loads
    mm("N = 1, M = 128 + 2, K = 16 + 4", 2, 130, 1, 20, 0, 0, 1, bias=1),
    mm("M < 16, K = 16 + 8", 2, 12, 48, 24, 0, 1, 1, bias=0, alpha=1.5),
    mm("N = 5, M = 128 + 4, K = 16 + 12", 2, 132, 5, 28, 1, 0, 1),
    mm("K = 3 on vector loads", 2, 48, 44, 3, 1, 1, 1, bias=0),
    mm("exact splits", 1, 48, 48, 1024, 0, 0, 1, 4),
    mm("exact splits", 2, 16, 48, 1024, 0, 1, 1, 4),
    mm("exact splits, N = 1", 1, 48, 1, 1024, 1, 0, 1, 4),
    mm("exact splits", 1, 44, 40, 1024, 1, 1, 1, 4),
    mm("ragged last split", 1, 40, 33, 1040, 0, 0, 1, 4),
    mm("ragged last split", 1, 12, 48, 1040, 0, 1, 1, 4),
    mm("ragged last split", 2, 48, 7, 1040, 1, 0, 1, 4),
    mm("ragged last split, odd K = 2049", 1, 48, 48, 2049, 1, 1, 1, 8),
    # -- tile 2, 128x96 vector loads (N % 96 == 0, N % 128 != 0); N = 192: two column tiles
    mm("M = 128 + 12", 1, 140, 96, 72, 0, 0, 2, alpha=2.0),
    mm("M < 16, two column tiles, K = 16", 2, 15, 192, 16, 0, 1, 2, bias=0),
    mm("M = 128 + 4, K = 8", 1, 132, 96, 8, 1, 0, 2, bias=1),
    mm("two row and two column tiles, K = 16 + 4", 1, 200, 192, 20, 1, 1, 2),
    mm("exact splits", 1, 16, 96, 1024, 0, 0, 2, 4),
    mm("exact splits, two column tiles", 1, 20, 192, 1024, 0, 1, 2, 4),
    mm("exact splits", 1, 48, 96, 1024, 1, 0, 2, 4),
    mm("exact splits", 2, 16, 96, 1024, 1, 1, 2, 4),
    mm("ragged last split", 1, 9, 96, 1040, 0, 0, 2, 4),
    mm("ragged last split", 1, 16, 96, 1040, 0, 1, 2, 4),
    mm("ragged last split", 1, 16, 96, 1040, 1, 0, 2, 4),
    mm("ragged last split, odd K = 2049", 1, 48, 96, 2049, 1, 1, 2, 8),
    # -- tile 3, 128x128 vector loads; N = 384 takes it (three column tiles) where N = 192 takes the 96-column tile
    mm("N = 48 + 1", 2, 37, 49, 24, 0, 0, 3),
    mm("N = 384 against N = 192", 1, 15, 384, 16, 0, 1, 3, bias=0),
    mm("N = 96 + 1, M = 128 + 8", 1, 136, 97, 28, 1, 0, 3),
    mm("N = 128 + 4, M = 128 + 8", 1, 136, 132, 72, 1, 1, 3, bias=1, alpha=0.125),
    mm("N = 128 + 1: the second column tile has one column", 1, 130, 129, 20, 0, 0, 3, bias=0),
    mm("exact splits, N = 64 + 1", 1, 16, 65, 1024, 0, 0, 3, 4),
    mm("exact splits", 1, 20, 128, 1024, 0, 1, 3, 4),
    mm("exact splits, N = 48 + 1", 1, 48, 49, 1024, 1, 0, 3, 4),
    mm("exact splits", 1, 48, 52, 1024, 1, 1, 3, 4),
    mm("ragged last split, N = 96 + 1", 1, 16, 97, 1040, 0, 0, 3, 4),
    mm("ragged last split", 1, 15, 100, 1040, 0, 1, 3, 4),
    mm("ragged last split", 1, 16, 128, 1040, 1, 0, 3, 4),
    mm("ragged last split, odd K = 2049, N = 128 + 4", 1, 16, 132, 2049, 1, 1, 3, 8),
]

# ---- other options --------------------------------------------------------------------------------------------------------
OPTION_CASES = [
    mm("shared B (stride_b = 0)", 3, 40, 52, 24, 0, 0, 3, stride_b=0, bias=0),
    mm("shared A (stride_a = 0)", 3, 40, 48, 20, 1, 1, 1, stride_a=0, bias=1),
    mm("shared B on the scalar tile", 3, 21, 10, 7, 0, 1, 0, stride_b=0),
    # bias, alpha and a strided / grouped C under split-K: the reduce kernel applies them, not the GEMM
    mm("split: bias[n], alpha, ldc > N, c_off", 2, 20, 48, 1040, 0, 1, 1, 4, ldc=61, c_off=7, bias=0, alpha=-0.5),
    mm("split: bias[m], alpha, grouped C", 1, 24, 96, 1040, 1, 1, 2, 4, ldb=32, Nc=32, gsbn=1040 * 32, ldc=40, gsc=24 * 40 + 8,
       c_off=3, bias=1, alpha=0.75),
    mm("split on the scalar tile: bias[n], alpha, ldc > N, grouped C", 1, 19, 39, 1041, 0, 1, 0, 4, ldb=13, Nc=13,
       gsbn=1041 * 13 + 5, ldc=17, gsc=19 * 17 + 2, c_off=1, bias=0, alpha=3.0),
    mm("split: k-groups, bias[m]", 1, 40, 36, 1040, 0, 0, 1, 4, lda=104, ldb=104, Kc=104, gsa=40 * 104 + 4, gsbk=36 * 104 + 8, bias=1),
]


# ---- head forms: the descriptors of ops.PositionAttention for h = 2, second head ---------------------------------------------
def head_cases(B, Tq, Tk, h, d, i, packed, tile):
    """the six contractions of PositionAttention.forward / backward for head i; dk = dv = d; packed: q | k side by side in
    rows of 2 * h * dk (then Tq == Tk)"""
    hd = h * d
    ldq = 2 * hd if packed else hd
    k_off, ldk = (hd, ldq) if packed else (0, hd)
    sS = h * Tq * Tk
    tag = f"h{h} d{d} head {i}" + (" packed" if packed else "")
    qk = [
        mm(f"S = q k^T, {tag}", B, Tq, Tk, d, 0, 0, tile, lda=ldq, ldb=ldk, ldc=Tk, stride_a=Tq * ldq, stride_b=Tk * ldk,
           stride_c=sS, a_off=i * d, b_off=k_off + i * d, c_off=i * Tq * Tk),
        mm(f"dq = dS k, {tag}", B, Tq, d, Tk, 0, 1, tile, lda=Tk, ldb=ldk, ldc=ldq, stride_a=sS, stride_b=Tk * ldk,
           stride_c=Tq * ldq, a_off=i * Tq * Tk, b_off=k_off + i * d, c_off=i * d),
        mm(f"dk = dS^T q, {tag}", B, Tk, d, Tq, 1, 1, tile, lda=Tk, ldb=ldq, ldc=ldk, stride_a=sS, stride_b=Tq * ldq,
           stride_c=Tk * ldk, a_off=i * Tq * Tk, b_off=i * d, c_off=k_off + i * d),
    ]
    if packed:
        return qk
    return qk + [
        mm(f"O = P v, {tag}", B, Tq, d, Tk, 0, 1, tile, lda=Tk, ldb=hd, ldc=hd, stride_a=sS, stride_b=Tk * hd, stride_c=Tq * hd,
           a_off=i * Tq * Tk, b_off=i * d, c_off=i * d),
        mm(f"dV = P^T dO, {tag}", B, Tk, d, Tq, 1, 1, tile, lda=Tk, ldb=hd, ldc=hd, stride_a=sS, stride_b=Tq * hd,
           stride_c=Tk * hd, a_off=i * Tq * Tk, b_off=i * d, c_off=i * d),
        mm(f"dP = dO v^T, {tag}", B, Tq, Tk, d, 0, 0, tile, lda=hd, ldb=hd, ldc=Tk, stride_a=Tq * hd, stride_b=Tk * hd,
           stride_c=sS, a_off=i * d, b_off=i * d, c_off=i * Tq * Tk),
    ]


# (B, Tq, Tk, h, dk = dv): d = 6 puts the second head 24 bytes into a row (scalar tile), d = 8 leaves it aligned (128x48)
HEAD_SHAPES = [(2, 20, 24, 2, 6, 0), (2, 20, 24, 2, 8, 1)]
HEAD_SHAPES_PACKED = [(2, 20, 20, 2, 6, 0), (2, 20, 20, 2, 8, 1)]
HEAD_CASES = ([c for B, Tq, Tk, h, d, t in HEAD_SHAPES for c in head_cases(B, Tq, Tk, h, d, 1, False, t)] +
              [c for B, Tq, Tk, h, d, t in HEAD_SHAPES_PACKED for c in head_cases(B, Tq, Tk, h, d, 1, True, t)])


# ---- group forms: the fc_o contractions of ops.ChannelAttention -------------------------------------------------------------
def group_cases(B, T, Cn, tile_n, tile_k, tile_1):
    """fc_o forward, weight gradient, data gradient and bias gradient over qn / yn [B][T][Cn]: n-groups of Cn columns (one per
    image) for the data paths, k-groups of Cn for the two parameter gradients"""
    tag = f"B{B} T{T} C{Cn}"
    one = dict(stride_a=0, stride_b=0, stride_c=0)        # batch = 1: ops.py leaves the batch strides at 0
    return [
        mm(f"fc_o forward (n-groups, bias[m]), {tag}", 1, T, B * Cn, T, 0, 1, tile_n, lda=T, ldb=Cn, ldc=Cn, Nc=Cn, gsbn=T * Cn,
           gsc=T * Cn, bias=1, **one),
        mm(f"fc_o weight gradient (k-groups), {tag}", 1, T, T, B * Cn, 0, 0, tile_k, lda=Cn, ldb=Cn, ldc=T, Kc=Cn, gsa=T * Cn,
           gsbk=T * Cn, **one),
        mm(f"fc_o data gradient (A cols, n-groups), {tag}", 1, T, B * Cn, T, 1, 1, tile_n, lda=T, ldb=Cn, ldc=Cn, Nc=Cn,
           gsbn=T * Cn, gsc=T * Cn, **one),
        mm(f"fc_o bias gradient (k-groups, N = 1), {tag}", 1, T, 1, B * Cn, 0, 0, tile_1, lda=Cn, ldb=B * Cn, ldc=1, Kc=Cn,
           gsa=T * Cn, gsbk=Cn, **one),
    ]


# C = 16: a group boundary inside the 48-column tile; C = 24: inside a 16-column fragment and a 16-element k stage (Kc = 24),
# N = 96 on the 128x96 tile; C = 6 with T = 13: the same on the scalar tile (Nc = Kc = 6, boundaries inside the float4 chunks)
GROUP_CASES = group_cases(3, 48, 16, 1, 1, 1) + group_cases(4, 20, 24, 2, 1, 1) + group_cases(3, 13, 6, 0, 0, 0)

# ---- hard operands: all 24 mantissa bits set, exponents spread over 2^40 (A) and 2^16 (B) inside a reduction, one per tile ---
HARD_CASES = [
    mm("hard operands", 2, 50, 67, 72, 1, 1, 0, hard=1),
    mm("hard operands", 2, 40, 48, 72, 0, 1, 1, hard=1),
    mm("hard operands", 1, 136, 96, 72, 0, 0, 2, hard=1),
    mm("hard operands", 1, 40, 132, 72, 1, 0, 3, hard=1),
    mm("hard operands, ragged last split", 1, 16, 48, 1040, 1, 1, 1, 4, hard=1),
]

CASES = FORM_CASES + OPTION_CASES + HEAD_CASES + GROUP_CASES + HARD_CASES

# ---- the search grid of the closure test (dense descriptors) ---------------------------------------------------------------
GRID_MN = [1, 15, 48, 49, 96, 97, 128, 192, 200, 384]
GRID_K = [3, 16, 20, 72, 1024, 1040, 2049]
GRID_BATCH = [1, 4]
GRID_OFF = [0, 1]          # a_off in elements: aligned / 4 bytes past alignment


def case_id(c):
    return (f"{LAYOUT[(c.a_layout, c.b_layout)]}-b{c.batch}-{c.M}x{c.N}x{c.K}-t{c.tile}{'s' if c.nsplit > 1 else ''}-"
            + c.name.replace(" ", "_"))


def desc(c):
    from buctd_amd import _C
    return _C.MatmulDesc(c.batch, c.M, c.N, c.K, c.a_layout, c.b_layout, c.lda, c.ldb, c.ldc, c.stride_a, c.stride_b, c.stride_c,
                         c.Kc, c.gsa, c.gsbk, c.Nc, c.gsbn, c.gsc, c.alpha, c.bias_axis or 0)


def plan(c, a_base=BASE, b_base=BASE):
    """buctd_matmul_plan as a dict of PLAN_FIELDS, or None where the launch would refuse the call; a_base / b_base: the byte
    addresses of the buffers the offsets of the case count from"""
    from buctd_amd import _C
    out = (C.c_int * len(PLAN_FIELDS))()
    d = desc(c)
    if _C.lib().buctd_matmul_plan(C.byref(d), a_base + 4 * c.a_off, b_base + 4 * c.b_off, out) != 0:
        return None
    return dict(zip(PLAN_FIELDS, out))


def plan_key(c, pl):
    """(layouts, tile, vec, K split, last split ragged)"""
    return (LAYOUT[(c.a_layout, c.b_layout)], pl["tile"], pl["vec"], pl["nsplit"] > 1,
            pl["nsplit"] > 1 and c.K % pl["k_per_split"] != 0)


# ---- operands, reference inputs and write set of a case ---------------------------------------------------------------------
def hard_operands(shape, g, lo, hi):
    from tests.test_gpu_conv3x3_plan_cover import hard_operands as gen
    return gen(shape, g, lo, hi, 0)


def addresses(c):
    """element addresses (from the start of each buffer, pointer offsets included) of A [batch][M][K], B [batch][K][N] and
    C [batch][M][N], by the formulas in the header comment of matmul.hip"""
    b = torch.arange(c.batch).view(-1, 1, 1)
    m, n, k = torch.arange(c.M), torch.arange(c.N), torch.arange(c.K)
    kg = k // c.Kc, k % c.Kc
    if c.a_layout == 0:
        a = m.view(1, -1, 1) * c.lda + (kg[0] * c.gsa + kg[1]).view(1, 1, -1)
    else:
        a = k.view(1, 1, -1) * c.lda + m.view(1, -1, 1)
    if c.b_layout == 0:
        bb = n.view(1, 1, -1) * c.ldb + (kg[0] * c.gsbk + kg[1]).view(1, -1, 1)
    else:
        bb = k.view(1, -1, 1) * c.ldb + ((n // c.Nc) * c.gsbn + n % c.Nc).view(1, 1, -1)
    cc = m.view(1, -1, 1) * c.ldc + ((n // c.Nc) * c.gsc + n % c.Nc).view(1, 1, -1)
    return (c.a_off + b * c.stride_a + a).expand(c.batch, c.M, c.K), (c.b_off + b * c.stride_b + bb).expand(c.batch, c.K, c.N), \
        c.c_off + b * c.stride_c + cc


Built = collections.namedtuple("Built", "A B bias a_buf b_buf c_addr c_len")


def build(c):
    """A [batch][M][K], B [batch][K][N] (fp64 copies of float values), bias (fp64 or None), the flat float buffers the kernel
    reads (every element that is no operand element is NaN: a read outside the operands poisons the result), the addresses
    [batch][M][N] of the elements of C the case writes, and the length of the C buffer"""
    g = torch.Generator().manual_seed(sum((i + 3) * int(v) for i, v in enumerate(c[1:22])) * 7 + 1)
    na, nb = (1 if c.stride_a == 0 else c.batch), (1 if c.stride_b == 0 else c.batch)
    if c.hard:
        A, B = hard_operands((na, c.M, c.K), g, -20, 20), hard_operands((nb, c.K, c.N), g, -8, 8)
    else:
        A = torch.randn(na, c.M, c.K, generator=g) + 0.5
        B = torch.randn(nb, c.K, c.N, generator=g) / math.sqrt(c.K)
    A, B = A.expand(c.batch, c.M, c.K), B.expand(c.batch, c.K, c.N)
    bias = None if c.bias_axis is None else torch.randn(c.M if c.bias_axis == 1 else c.N, generator=g)
    a_addr, b_addr, c_addr = addresses(c)
    assert c_addr.unique().numel() == c_addr.numel() and int(c_addr.min()) >= 0, f"{case_id(c)}: C elements overlap"
    bufs = []
    for val, addr, shared in ((A, a_addr, c.stride_a == 0), (B, b_addr, c.stride_b == 0)):
        assert int(addr.min()) >= 0
        if not shared:
            assert addr.unique().numel() == addr.numel(), f"{case_id(c)}: operand elements overlap"
        buf = torch.full((int(addr.max()) + 1,), float("nan"), dtype=torch.float32)
        buf[addr.reshape(-1)] = val.reshape(-1)
        bufs.append(buf)
    return Built(A.double(), B.double(), None if bias is None else bias.double(), bufs[0], bufs[1], c_addr, int(c_addr.max()) + 1)
