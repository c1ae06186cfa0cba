"""The case table of the fused narrow-contraction attention (csrc/attn_smallqk.hip), as data, with its fp64 references.

A case is one call of the C entry points buctd_attn_smallqk_fwd / _bwd: (B, T, R4, C), the math flag (0 fp32 MFMA, 1 two bf16
pieces, 2 three), p_drop and an input family.  q' and k' are dense over all R4 columns (the model's q' has zero pad columns:
there a kernel that dropped a column would pass).  route(case) is what buctd_attn_smallqk_plan reports for it: the GPU test
asserts the route before it runs, tests/test_attn_plan_cover.py (host only) proves that the table reaches every route and
every attn_launch<R4, CF> instance, and that the input families are what they claim to be.

Shapes, the smallest at which each thing can go wrong: T = 64 is one key tile and one workgroup per image, T = 128 two of
each, T = 576 a 512-key chunk of attn_stats_kernel plus a 64-key tail and a partial last 256-row block; B = 2 so that the
image offset and the dropout row key b*T + i matter.

Input families:
  gaussian  q', k' ~ N(0, 1)
  rising    the logits of every query row grow along the key index by more than their noise per 64-key tile: the row maximum
            moves in every tile (the rescale of attn_fwd_b3_kernel and the s > mx branch of attn_stats_kernel run throughout)
  falling   the mirror image: the maximum is fixed in tile 0
  peaked    every row puts >= 0.99 of its probability on one key (R4 groups of rows, one key each, logits about -h / +h,
            h = 4.6 ... 5.7)
"""
import collections
import ctypes as C
import functools
import math

import torch

R4S = (4, 8, 16, 20)
CS = (16, 32, 48, 64, 96, 128, 192)
FLAGS = (0, 1, 2)
TS = (64, 128, 576)
P_DROP = 0.3
SEED = 0xC0FFEE1234567ABC           # the two 32-bit halves differ: the kernels key rows by one and columns by the other
FAMILIES = ("gaussian", "rising", "falling", "peaked")
PLAN_FIELDS = ("split", "R4", "CF", "pieces", "stats", "drop", "dseed")
B = 2

Case = collections.namedtuple("Case", "T R4 C flag p inputs")

# nine key tiles: rising on each kernel family and piece count, the other families spread over the rest
T576_INPUTS = {(4, 0): "rising", (4, 1): "peaked", (4, 2): "rising", (8, 0): "falling", (8, 1): "rising", (8, 2): "gaussian",
               (16, 0): "peaked", (16, 1): "gaussian", (16, 2): "rising", (20, 0): "gaussian", (20, 1): "falling",
               (20, 2): "peaked"}


def _table():
    cases = []
    for ir, r4 in enumerate(R4S):
        for ic, c in enumerate(CS):
            for flag in FLAGS:
                # the four families go round over (R4, C) and over the three slots of a (R4, C, flag): with R4 in {4, 8} alone
                # (the split kernels) every (pieces, CF) still meets all four
                fam = lambda slot: FAMILIES[(ir + ic + slot) % 4]
                cases.append(Case(128, r4, c, flag, 0.0, fam(0)))
                cases.append(Case(128, r4, c, flag, P_DROP, fam(2)))
                cases.append(Case(64, r4, c, flag, P_DROP if (ir + ic) % 2 else 0.0, fam(1)))
    for ir, r4 in enumerate(R4S):
        for flag in FLAGS:
            cases.append(Case(576, r4, CS[(3 * ir + flag) % 7], flag, P_DROP if (ir + flag) % 2 else 0.0, T576_INPUTS[(r4, flag)]))
    return cases


CASES = _table()


def case_id(c):
    return f"T{c.T}-R{c.R4}-C{c.C}-f{c.flag}-p{c.p:g}-{c.inputs}"


def plan(T, R4, Cn, flag, p, dseed):
    """buctd_attn_smallqk_plan as a dict of PLAN_FIELDS, or None where the launch would refuse the call"""
    from buctd_amd import _C
    out = (C.c_int * len(PLAN_FIELDS))()
    if _C.lib().buctd_attn_smallqk_plan(T, R4, Cn, flag, p, int(dseed), out) != 0:
        return None
    return dict(zip(PLAN_FIELDS, out))


def route(c, dseed=False):
    return plan(c.T, c.R4, c.C, c.flag, c.p, dseed)


def route_key(pl):
    return tuple(pl[f] for f in PLAN_FIELDS)


def scale_of(c):
    return 1.0 / math.sqrt(c.C)


# ---- operands -------------------------------------------------------------------------------------------------------------
RISE_STEP = 2.5         # growth of the ramp per 64-key tile; the noise of a logit has std 0.25 before the scale (below)
PEAK_REST = 0.006       # peaked: the probability a row leaves to all other keys together.  Just past the 0.99 the family
                        # promises: dS = P (dP - sum P dP) cancels to 1 / PEAK_REST of its terms, and a sharper peak would
                        # leave the gradients to fp32 round-off (bars of per cent, which test nothing)


def peak_logit(T):
    """the row's key at +h, every other key at -h, (T - 1) exp(-2h) = PEAK_REST"""
    return 0.5 * math.log((T - 1) / PEAK_REST)


def peak_keys(T, R4):
    """the key of each of the R4 row groups of the peaked family: distinct (77 is coprime to every T) and spread over the tiles"""
    return [(5 + 77 * g) % T for g in range(R4)]


@functools.lru_cache(maxsize=None)
def operands(c):
    """q', k' [B][T][R4], v, dout [B][T][C]: float32 values (the kernels' operands), deterministic per case"""
    g = torch.Generator().manual_seed(c.T * 1009 + c.R4 * 101 + c.C * 7 + c.flag * 3 + int(c.p > 0) + 11)
    T, R4 = c.T, c.R4
    rn = lambda *s: torch.randn(*s, generator=g)
    if c.inputs == "gaussian":
        q, k = rn(B, T, R4), rn(B, T, R4)
    elif c.inputs in ("rising", "falling"):
        # logit / scale = q0 ramp(j) + noise, q0 >= 1, noise ~ 0.25 N(0, 1): a tile's gain RISE_STEP q0 beats twice the noise range
        q = 0.5 * rn(B, T, R4)
        q[:, :, 0] = 1.0 + 0.5 * rn(B, T).abs()
        k = 0.5 * rn(B, T, R4) / math.sqrt(R4 - 1)
        ramp = RISE_STEP * (torch.arange(T, dtype=torch.float32) - (T - 1) / 2) / 64
        k[:, :, 0] = ramp if c.inputs == "rising" else ramp.flip(0)
    else:
        # rows of group g have q' ~ A e_g; k'[j][g] = +A at the group's key, -A elsewhere; scale A^2 = peak_logit(T)
        A = math.sqrt(peak_logit(T) / scale_of(c))
        group = torch.stack([(torch.arange(T) % R4)[torch.randperm(T, generator=g)] for _ in range(B)])    # every group, shuffled
        q = 0.02 * rn(B, T, R4) + A * torch.nn.functional.one_hot(group, R4).float()
        k = 0.02 * rn(B, T, R4) - A
        for grp, j in enumerate(peak_keys(T, R4)):
            k[:, j, grp] += 2 * A
    v, dout = rn(B, T, c.C), rn(B, T, c.C)
    return tuple(t.float().contiguous() for t in (q, k, v, dout))


@functools.lru_cache(maxsize=None)
def keep(c):
    """the dropout mask of the case as 0 / 1 in fp64 [B][T][T] (None without dropout): the host mirror of the kernels' hash"""
    if c.p == 0:
        return None
    from tests.helpers.dropout_mask import keep_mask
    return torch.from_numpy(keep_mask(SEED, B, c.T, c.p)).double()


NAMES = ("out", "lse", "dq", "dk", "dv", "dvec")      # what is compared; m / linv enter through the log-sum-exp they encode


def formulas(c, dtype):
    """the formulas of the issue in plain torch at `dtype` on the CPU -> dict over NAMES plus P (the soft-max matrix)"""
    q, k, v, dout = (t.to(dtype) for t in operands(c))
    scale = scale_of(c)
    s = scale * torch.matmul(q, k.transpose(1, 2))
    P = torch.softmax(s, -1)
    mask = keep(c)
    w = None if mask is None else mask.to(dtype) / (1.0 - c.p)
    Pd = P if w is None else P * w
    out = torch.matmul(Pd, v)
    dv = torch.matmul(Pd.transpose(1, 2), dout)
    dP = torch.matmul(dout, v.transpose(1, 2))
    dvec = (dout * out).sum(-1)
    dS = P * ((dP if w is None else dP * w) - dvec.unsqueeze(-1))
    return {"out": out, "lse": torch.logsumexp(s, -1), "dq": scale * torch.matmul(dS, k),
            "dk": scale * torch.matmul(dS.transpose(1, 2), q), "dv": dv, "dvec": dvec, "P": P, "s": s}


@functools.lru_cache(maxsize=None)
def reference(c):
    """fp64; computed once per case and shared: do not modify"""
    return formulas(c, torch.float64)


def lse_of(m, linv):
    """natural log-sum-exp of the scaled logits from the saved statistics: attn_stats_kernel keeps m in the exp2 domain
    (m = max_j scale log2(e) q'.k'_j, linv = 1 / sum_j exp2(s_j - m)), so lse = m ln 2 - ln(linv) whichever maximum was kept"""
    return m.double() * math.log(2.0) - linv.double().log()


def errors(got, ref):
    """(relative L2 over the tensor, max-abs error over max-abs of the reference)"""
    got, ref = got.double().cpu(), ref.double()
    d = got - ref
    return (d.norm() / ref.norm()).item(), (d.abs().max() / ref.abs().max()).item()


PROJECT_BAR = {0: 2e-5, 2: 5e-5, 3: 2e-5}      # by bf16 pieces: fp32 MFMA, two pieces (bf16x3 class), three (fp32 class)


@functools.lru_cache(maxsize=None)
def fp32_errors(c):
    """{name: (rel L2, max-abs ratio)} of the plain fp32 torch evaluation of the same formulas against fp64"""
    lo, ref = formulas(c, torch.float32), reference(c)
    return {n: errors(lo[n], ref[n]) for n in NAMES}


def bars(c, pieces):
    """{name: (bar on the relative L2, bar on the max-abs ratio)}.  gaussian: the project's stated bar.  The other families:
    no bar can be derived in advance (cancellation in dS for near one-hot rows, large logits), so each is max(project bar,
    4 x the error of the fp32 evaluation above in that norm): 4 covers another summation order plus one more rounding per
    rescaled tile.  Never from the kernel."""
    base = PROJECT_BAR[pieces]
    if c.inputs == "gaussian":
        return {n: (base, base) for n in NAMES}
    lo = fp32_errors(c)
    return {n: (max(base, 4.0 * lo[n][0]), max(base, 4.0 * lo[n][1])) for n in NAMES}


def dseed_cases():
    """the cases whose device-seed form the GPU test runs beside the value-seed form: every (R4, C, flag) with dropout"""
    return [c for c in CASES if c.T == 128 and c.p > 0]
