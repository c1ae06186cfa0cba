"""The case table of the bf16x6 GEMM tests (csrc/gemm_x6.hip: x6_image_kernel + x6_gemm_kernel), as data.

A case is a product M x N x K, the address functions of both operands as buctd_x6_image takes them (Addr: the element
X[v][k] sits at src[off + (v // vg) * vgs + (v % vg) * vs + (k // kg) * kgs + (k % kg) * ks], vg / kg = 0: plain strides;
v = m for the A operand, v = n for the B operand), the epilogue as buctd_x6_gemm takes it (Epi: C(m, n) = C[c_off + m * ldc +
(n // Nc) * gsc + n % Nc], Nc = 0: no grouping; bias axis 0 = bias[n], 1 = bias[m], None = no bias; alpha), whether the
operands are the hard ones, and - for the grid-order cases - the (grid x, grid y, row_major) that buctd_x6_gemm_plan must report.

tests/test_gemm_x6_plan_cover.py (host only) proves that the table reaches every workgroup order, every branch of the XCD remap,
both load paths of the image kernel in both roles and every epilogue form that occur on the search grid below, and that the
remap is a bijection; tests/test_gpu_gemm_x6_paths.py runs every case against fp64.  build() makes the operands and the write
set from the two formulas above alone, so the reference shares no argument handling with ops.x6_image / ops.x6_gemm.

The workgroup tile is 128 x 192 and K is padded to 256, so the grid-order cases need many tiles, not a large K: all have K = 8.
M = N = 1152 is a 9 x 6 grid whose two padded extents are EQUAL, and the launch takes the row-major order only where the
padded M is larger - it runs column-major, and the table says so; 54 workgroups in row-major order come from 18 x 3 instead."""
import collections
import ctypes as C
import math

import torch

BM, BN, KPAD = 128, 192, 256
PLAN_FIELDS = ("gx", "gy", "row_major", "KB", "chunks", "total", "per", "rem")
# the base address plan queries give to a source: 16-byte aligned, like every allocation of the caching allocator
BASE = 1 << 20

Addr = collections.namedtuple("Addr", "vs ks vg vgs kg kgs off")
Epi = collections.namedtuple("Epi", "ldc c_off Nc gsc bias_axis alpha")
Case = collections.namedtuple("Case", "name group M N K a b epi hard grid")


# ---- address functions of a logical matrix X[V][K] ---------------------------------------------------------------------------
def contig(V, K, off=0):
    """[V][K], k contiguous: every full group of 8 on the two 16-byte loads where K % 4 == 0 (and off % 4 == 0)"""
    return Addr(K, 1, 0, 0, 0, 0, off)


def transposed(V, K, off=0):
    """stored [K][V] (ks = ld): gathered"""
    return Addr(1, V, 0, 0, 0, 0, off)


def odd_rows(V, K, off=0):
    """[V][ld] with an odd ld >= K + 1 and ks = 1: the rows alternate between the two load paths"""
    return Addr(K + 1 + K % 2, 1, 0, 0, 0, 0, off)


def vgrouped(V, K, g, off=0):
    """token-major activations [ceil(V / g)][K][g]: v = (group, channel), the layout of the fc_o data operands"""
    return Addr(1, g, g, K * g, 0, 0, off)


def kgrouped(V, K, g, off=0):
    """[ceil(K / g)][V][g]: k = (group, channel), the layout of the fc_o weight-gradient operands"""
    return Addr(g, 1, 0, 0, g, V * g, off)


def plain(N, bias=None, alpha=1.0):
    return Epi(N, 0, 0, 0, bias, alpha)


def gx(name, group, M, N, K, a=None, b=None, epi=None, hard=0, grid=None):
    """a case; what is not given: A [M][K] contiguous, B stored [K][N] (the transposed form), C [M][N] dense, no bias"""
    return Case(name, group, M, N, K, contig(M, K) if a is None else a, transposed(N, K) if b is None else b,
                plain(N) if epi is None else epi, hard, grid)


# ---- workgroup order: grid x, grid y, row_major as the plan must report them; K = 8 ----------------------------------------
GRID_CASES = [
    gx("1 workgroup", "grid", 100, 150, 8, grid=(1, 1, 0)),
    gx("3 x 1, fewer than 8", "grid", 384, 192, 8, grid=(3, 1, 1), epi=plain(192, 0)),
    gx("4 x 2 = 8: per 1, rem 0", "grid", 512, 384, 8, grid=(4, 2, 1)),
    gx("5 x 3 = 15: per 1, rem 7", "grid", 640, 576, 8, grid=(5, 3, 1), epi=plain(576, 1)),
    gx("3 x 5 = 15: per 1, rem 7", "grid", 384, 960, 8, grid=(3, 5, 0), epi=plain(960, 0, 0.5)),
    gx("9 x 6 = 54: per 6, rem 6, equal padded extents", "grid", 1152, 1152, 8, grid=(9, 6, 0)),
    gx("18 x 3 = 54: per 6, rem 6", "grid", 2304, 576, 8, grid=(18, 3, 1), epi=plain(576, 1)),
    gx("6 x 9 = 54: per 6, rem 6", "grid", 768, 1728, 8, grid=(6, 9, 0), epi=plain(1728, 0)),
    gx("8 x 2 = 16: per 2, rem 0", "grid", 1024, 384, 8, grid=(8, 2, 1)),
    gx("4 x 4 = 16: per 2, rem 0", "grid", 512, 768, 8, grid=(4, 4, 0)),
    # ragged last tiles under both orders with more than 8 workgroups
    gx("5 x 3 ragged", "grid", 513, 385, 8, grid=(5, 3, 1), epi=plain(385, 0)),
    gx("3 x 4 ragged", "grid", 257, 577, 8, grid=(3, 4, 0), epi=plain(577, 1)),
]

# ---- tails: a wave wholly past the edge (1, 15, 16, 17 of a 64 x 48 wave tile), partly past it, one row / column into a tile -
TAIL_MN = [(1, 1, 1), (1, 193, 9), (15, 191, 8), (16, 129, 9), (17, 127, 33), (127, 17, 8), (129, 16, 9), (191, 15, 33),
           (193, 1, 8), (129, 193, 7)]
TAIL_CASES = [gx("edge", "tail", M, N, K, epi=plain(N, (None, 0, 1)[i % 3])) for i, (M, N, K) in enumerate(TAIL_MN)]
# K: the tail inside a group of 8, inside a 32-slot block and inside the 256 padding; 257 and 513 give two and three trips of the
# four-chunk loop.  Both operands k-contiguous (K % 4 != 0: the rows alternate between the load paths), then both gathered.
TAIL_K = [1, 7, 8, 9, 31, 33, 255, 256, 257, 513]
TAIL_CASES += [gx("K tail, k-contiguous operands", "tail", 33, 20, K, b=contig(20, K)) for K in TAIL_K]
TAIL_CASES += [gx("K tail, transposed operands", "tail", 33, 20, K, a=transposed(33, K)) for K in (1, 7, 257)]

# ---- address functions, each as the A operand and as the B operand; ragged groups: 70 = 5 * 12 + 10 = 3 * 20 + 10 = 48 + 22,
# 50 = 4 * 12 + 2 = 2 * 20 + 10 = 48 + 2, 52 = 4 * 12 + 4 = 2 * 20 + 12 = 48 + 4 -------------------------------------------
AM, AN, AK = 70, 50, 52
ADDR_FORMS = ([("contiguous", contig), ("transposed", transposed), ("odd vs", odd_rows)] +
              [(f"v-groups of {g}", lambda V, K, off=0, g=g: vgrouped(V, K, g, off)) for g in (12, 20, 48)] +
              [(f"k-groups of {g}", lambda V, K, off=0, g=g: kgrouped(V, K, g, off)) for g in (12, 20, 48)] +
              [(f"off {o}", lambda V, K, off=0, o=o: contig(V, K, o)) for o in (1, 2, 3, 4)] +
              [("transposed off 3", lambda V, K, off=0: transposed(V, K, 3)),
               ("odd vs off 1", lambda V, K, off=0: odd_rows(V, K, 1)),
               ("k-groups of 12 off 2", lambda V, K, off=0: kgrouped(V, K, 12, 2))])
ADDR_CASES = ([gx(f"A {n}", "addr", AM, AN, AK, a=f(AM, AK), b=contig(AN, AK)) for n, f in ADDR_FORMS] +
              [gx(f"B {n}", "addr", AM, AN, AK, b=f(AN, AK)) for n, f in ADDR_FORMS])


# ---- the three fc_o products of ops.ChannelAttention on token-major activations [B][T][Cn] ---------------------------------
def fc_o_cases(B, T, Cn):
    tag = f"B{B} T{T} C{Cn}"
    grouped = Epi(Cn, 0, Cn, T * Cn, None, 1.0)
    return [
        gx(f"fc_o forward, {tag}", "fc_o", T, B * Cn, T, a=contig(T, T), b=vgrouped(B * Cn, T, Cn), epi=grouped._replace(bias_axis=1)),
        gx(f"fc_o data gradient, {tag}", "fc_o", T, B * Cn, T, a=transposed(T, T), b=vgrouped(B * Cn, T, Cn), epi=grouped),
        gx(f"fc_o weight gradient, {tag}", "fc_o", T, T, B * Cn, a=kgrouped(T, B * Cn, Cn), b=kgrouped(T, B * Cn, Cn)),
    ]


FC_O_CASES = fc_o_cases(3, 160, 48) + fc_o_cases(3, 160, 20)          # N = 144, and N = 60: no multiple of 16

# ---- epilogue forms on 2 x 2 tiles with ragged edges: 203 = 4 * 48 + 11 = 10 * 20 + 3 ---------------------------------------
EM, EN, EK = 137, 203, 40
EPI_CASES = [gx(f"bias {('none', 'per column', 'per row')[0 if ax is None else ax + 1]}, alpha {al}", "epi", EM, EN, EK,
                epi=plain(EN, ax, al)) for ax in (None, 0, 1) for al in (1.0, -0.75)]
EPI_CASES += [
    gx("ldc = N + 5", "epi", EM, EN, EK, epi=Epi(EN + 5, 0, 0, 0, 0, 1.0)),
    gx("c_off = 7", "epi", EM, EN, EK, epi=Epi(EN, 7, 0, 0, None, 1.0)),
    gx("ldc = N + 5, c_off = 3, bias per row, alpha", "epi", EM, EN, EK, epi=Epi(EN + 5, 3, 0, 0, 1, 2.5)),
    gx("column groups of 48, the last of 11", "epi", EM, EN, EK, epi=Epi(48 + 3, 3, 48, EM * 51 + 2, 1, 0.5)),
    gx("column groups of 20, the last of 3", "epi", EM, EN, EK, epi=Epi(20, 0, 20, EM * 20, 0, 1.0)),
]

# ---- hard operands: all 24 mantissa bits set, magnitudes over 2^+-12 inside one reduction ----------------------------------
HARD_CASES = [
    gx("hard operands, one full tile", "hard", 128, 192, 256, hard=1),
    gx("hard operands, ragged, two trips", "hard", 129, 193, 257, hard=1, epi=plain(193, 1, -0.75)),
    gx("hard operands, fc_o forward layout", "hard", 160, 60, 160, a=contig(160, 160), b=vgrouped(60, 160, 20),
       epi=Epi(20, 0, 20, 160 * 20, 1, 1.0), hard=1),
]

CASES = GRID_CASES + TAIL_CASES + ADDR_CASES + FC_O_CASES + EPI_CASES + HARD_CASES
GROUPS = ("grid", "tail", "addr", "fc_o", "epi", "hard")

# ---- the search grid of the closure test --------------------------------------------------------------------------------------
GRID_M = [1, 100, 128, 129, 384, 512, 640, 768, 1024, 1152, 1280, 2304]
GRID_N = [1, 150, 192, 193, 384, 576, 768, 960, 1152, 1728]
GRID_K = [1, 7, 8, 9, 52, 256, 257]
GRID_V = [1, 33]
GRID_ADDR = [("contiguous", contig), ("transposed", transposed), ("odd vs", odd_rows),
             ("v-groups", lambda V, K, off=0: vgrouped(V, K, 12, off)), ("k-groups", lambda V, K, off=0: kgrouped(V, K, 12, off))]
GRID_OFF = [0, 1, 2, 3, 4]


def case_id(c):
    return f"{c.group}-{c.M}x{c.N}x{c.K}-" + c.name.replace(" ", "_").replace(",", "")


# ---- the host-only queries --------------------------------------------------------------------------------------------------
def plan(M, N, K):
    """buctd_x6_gemm_plan as a dict of PLAN_FIELDS, or None where the launch would refuse the sizes"""
    from buctd_amd import _C
    out = (C.c_int * len(PLAN_FIELDS))()
    if _C.lib().buctd_x6_gemm_plan(M, N, K, out) != 0:
        return None
    return dict(zip(PLAN_FIELDS, out))


def tile_of(lin, gx_, gy, row_major):
    from buctd_amd import _C
    bx, by = C.c_int(-1), C.c_int(-1)
    assert _C.lib().buctd_x6_gemm_tile(lin, gx_, gy, row_major, C.byref(bx), C.byref(by)) == 0
    return bx.value, by.value


def order_key(pl):
    """(row_major, branch of the XCD remap): fewer than 8 workgroups (every xcd >= rem has no tile); a multiple of 8; ragged
    (xcd < rem and xcd >= rem both hold tiles, per > 0)"""
    return (pl["row_major"], "total < 8" if pl["per"] == 0 else "rem == 0" if pl["rem"] == 0 else "xcd < rem and xcd >= rem, per > 0")


def image_dims(V, K, role):
    from buctd_amd import _C
    vp, kp = C.c_int(), C.c_int()
    assert _C.lib().buctd_x6_image_dims(V, K, role, C.byref(vp), C.byref(kp)) == 0
    return vp.value, kp.value


def image_paths(ad, V, K, role, base=BASE):
    """{(v, k0): 1 vector / 0 gather} for every lane that holds an element (v < V, k0 < K), as buctd_x6_image_path reports it
    for a source allocation at byte address `base`"""
    from buctd_amd import _C
    fn = _C.lib().buctd_x6_image_path
    vec = C.c_int()
    out = {}
    src = base + 4 * ad.off
    for v in range(V):
        for k0 in range(0, K, 8):
            assert fn(src, V, K, ad.vg, ad.vgs, ad.vs, ad.kg, ad.kgs, ad.ks, role, v, k0, C.byref(vec)) == 0
            out[(v, k0)] = vec.value
    return out


def image_forms(ad, V, K, role, base=BASE):
    """the load forms an image call takes, by role: the two 16-byte loads; a gather and why (a k stride, k groups, the K tail
    inside a group of 8, an address off the 16-byte grid); rows that alternate between the two"""
    paths = image_paths(ad, V, K, role, base)
    forms = set()
    rows = {}
    for (v, k0), vec in paths.items():
        if k0 + 8 <= K:
            rows.setdefault(v, set()).add(vec)
        if vec:
            forms.add((role, "vector"))
        elif ad.kg:
            forms.add((role, "gather: k groups"))
        elif ad.ks != 1:
            forms.add((role, "gather: k stride"))
        elif k0 + 8 > K:
            forms.add((role, "gather: K tail inside a group of 8"))
        else:
            forms.add((role, "gather: address not on 16 bytes"))
    if {frozenset(s) for s in rows.values()} >= {frozenset({0}), frozenset({1})}:
        forms.add((role, "rows alternate"))
    return forms


def epi_forms(c):
    e = c.epi
    forms = {("bias", "none" if e.bias_axis is None else ("per column", "per row")[e.bias_axis], "alpha" if e.alpha != 1 else "1")}
    if e.ldc > (e.Nc or c.N):
        forms.add(("ldc > N",))
    if e.c_off:
        forms.add(("c_off",))
    if e.Nc and c.N % e.Nc:
        forms.add(("column groups, the last ragged", "N % 16" if c.N % 16 else "N % 16 == 0"))
    return forms


EPI_FORMS = ({("bias", b, a) for b in ("none", "per column", "per row") for a in ("1", "alpha")} |
             {("ldc > N",), ("c_off",), ("column groups, the last ragged", "N % 16")})


# ---- operands, reference inputs and write set of a case --------------------------------------------------------------------
def addresses(ad, V, K):
    """element offsets [V][K] from the start of the source buffer"""
    v, k = torch.arange(V).view(-1, 1), torch.arange(K).view(1, -1)
    vo = (v // ad.vg) * ad.vgs + (v % ad.vg) * ad.vs if ad.vg else v * ad.vs
    ko = (k // ad.kg) * ad.kgs + (k % ad.kg) * ad.ks if ad.kg else k * ad.ks
    return ad.off + vo + ko


def c_addresses(c):
    e = c.epi
    m, n = torch.arange(c.M).view(-1, 1), torch.arange(c.N).view(1, -1)
    return e.c_off + m * e.ldc + ((n // e.Nc) * e.gsc + n % e.Nc if e.Nc else n)


def hard_operands(shape, g, lo, hi, shift=0):
    from tests.test_gpu_conv3x3_plan_cover import hard_operands as gen
    return gen(shape, g, lo, hi, shift)


def source(X, ad):
    """the flat float buffer buctd_x6_image reads X [V][K] from; every element that is no element of X is NaN, so a read
    outside the matrix poisons the image"""
    addr = addresses(ad, *X.shape)
    assert int(addr.min()) >= 0 and addr.unique().numel() == addr.numel(), "operand elements overlap"
    buf = torch.full((int(addr.max()) + 1,), float("nan"), dtype=torch.float32)
    buf[addr.reshape(-1)] = X.reshape(-1)
    return buf


Built = collections.namedtuple("Built", "A B bias a_buf b_buf c_addr c_len")


def build(c):
    """A [M][K], B [K][N] (float), bias (float or None), the two source buffers, the addresses [M][N] of the elements of C the
    case writes, and the length of the C buffer"""
    g = torch.Generator().manual_seed((c.M * 131 + c.N) * 137 + c.K * 7 + sum(int(abs(x)) for x in c.a + c.b) % 1000 + 1)
    if c.hard:
        A, B = hard_operands((c.M, c.K), g, -12, 12), hard_operands((c.K, c.N), g, -12, 12)
    else:
        A = torch.randn(c.M, c.K, generator=g) + 0.5
        B = torch.randn(c.K, c.N, generator=g) / math.sqrt(c.K)
    bias = None if c.epi.bias_axis is None else torch.randn(c.M if c.epi.bias_axis == 1 else c.N, generator=g)
    c_addr = c_addresses(c)
    assert c_addr.unique().numel() == c_addr.numel() and int(c_addr.min()) >= 0, f"{case_id(c)}: C elements overlap"
    return Built(A, B, bias, source(A, c.a), source(B.t().contiguous(), c.b), c_addr, int(c_addr.max()) + 1)


# ---- the image format, from the header comment of gemm_x6.hip --------------------------------------------------------------
def decode_image(img, V, K, role):
    """fp64 [3][Vpad][Kpad] from the bytes of an image: block (vb, kb) = [3 pieces][64 lanes][8 bf16], lane l holds row
    vb * 16 + (l & 15), slots kb * 32 + (l >> 4) * 8 ..; blocks [Vpad / 16][Kpad / 32], k fastest.  Also the raw bf16 bit patterns."""
    vp, kp = image_dims(V, K, role)
    assert img.numel() == (vp // 16) * (kp // 32) * 3072
    bits = img.cpu().view(torch.int16).view(vp // 16, kp // 32, 3, 4, 16, 8)        # vb kb piece (l >> 4) (l & 15) e
    bits = bits.permute(2, 0, 4, 1, 3, 5).reshape(3, vp, kp)                          # piece, vb * 16 + i16, kb * 32 + g * 8 + e
    val = (bits.to(torch.int32) << 16).view(torch.float32).double()
    return val, bits
