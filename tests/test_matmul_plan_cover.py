"""Closure of the fp32 matmul case table (tests/helpers/matmul_cases.py) over the launch forms of matmul.hip (host only:
buctd_matmul_plan runs the routing function of buctd_matmul and mm_split_plan without a launch).

Every (layouts, tile, vec, K split, ragged last split) that mm_route / mm_split_plan can pick on the search grid must be
reached by a case of the table - so a retuned threshold or a new tile without a test shape fails here, by name - and every
launch_mm instance in the source is either reached or listed in UNREACHED with the reason."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

from tests.helpers import matmul_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "buctd_amd", "csrc", "matmul.hip")

# launch forms (keys of T.plan_key) that the grid finds and no case reaches, and why.  The only place where forms are left out.
UNREACHED = {}

EINVAL, EWORKSPACE = -1, -3


def instance(c, pl):
    """the template instance a plan launches: (A cols, B cols, WM, WN, MF, NF, vec)"""
    wn = 4 // pl["WM"]
    assert pl["BM"] == pl["WM"] * pl["MF"] * 16 and pl["BN"] % (wn * 16) == 0, pl
    return (c.a_layout, c.b_layout, pl["WM"], wn, pl["MF"], pl["BN"] // (wn * 16), pl["vec"])


def grid():
    for M, N, K, batch, (al, bl), off in itertools.product(T.GRID_MN, T.GRID_MN, T.GRID_K, T.GRID_BATCH, T.LAYOUT, T.GRID_OFF):
        yield T.mm("grid", batch, M, N, K, al, bl, None, None, a_off=off)


@pytest.fixture(scope="module")
def grid_plans():
    """{key: (first grid case, plan)} over the grid"""
    found = {}
    n = 0
    for c in grid():
        n += 1
        pl = T.plan(c)
        assert pl is not None, c
        found.setdefault(T.plan_key(c, pl), (c, pl))
    assert n == 10 * 10 * 7 * 2 * 4 * 2
    return found


def table_plans():
    return [(c, T.plan(c)) for c in T.CASES]


def test_every_case_reports_the_plan_the_table_names():
    ids = [T.case_id(c) for c in T.CASES]
    assert len(set(ids)) == len(ids), "case ids repeat"
    for c, pl in table_plans():
        assert pl is not None, f"{T.case_id(c)}: the launch would refuse the case"
        assert (pl["tile"], pl["vec"], pl["nsplit"]) == (c.tile, int(c.tile != 0), c.nsplit), f"{T.case_id(c)}: {pl}"
        assert pl["BM"] == 128 and pl["BN"] == (64, 48, 96, 128)[pl["tile"]], f"{T.case_id(c)}: {pl}"
        kps, ns = pl["k_per_split"], pl["nsplit"]
        assert kps % 16 == 0 and (ns - 1) * kps < c.K <= ns * kps, f"{T.case_id(c)}: {pl}"
    # the forms the issue names, by what makes them what they are
    scalar = [c for c in T.CASES if c.tile == 0]
    dense = lambda c: (c.lda, c.ldb) == (c.K if c.a_layout == 0 else c.M, c.K if c.b_layout == 0 else c.N) and c.Kc == c.K and c.Nc == c.N
    assert any(c.K % 2 and c.M % 2 and c.N % 2 for c in scalar), "scalar tile by odd sizes"
    assert any(c.lda % 2 and not (c.M % 4 or c.N % 4 or c.K % 4 or c.a_off or c.b_off) for c in scalar), "scalar tile by an odd lda"
    misaligned = [c for c in scalar if dense(c) and not (c.M % 4 or c.N % 4 or c.K % 4) and (c.a_off % 4 or c.b_off % 4)]
    assert misaligned, "scalar tile by a misaligned pointer alone"
    for c in misaligned:
        assert T.plan(c._replace(a_off=0, b_off=0))["vec"] == 1, T.case_id(c)
    assert any(c.nsplit > 1 and c.K % 2 for c in scalar), "split on the scalar tile with odd K"
    assert any(128 < c.M < 144 for c in T.CASES) and any(c.M < 16 for c in T.CASES)
    assert {1, 49, 65, 97, 129, 192, 384} <= {c.N for c in T.CASES} and {3, 16, 20, 24, 28, 72} <= {c.K for c in T.CASES}
    assert {T.plan(c)["tile"] for c in T.CASES if c.N == 192} == {2} and {T.plan(c)["tile"] for c in T.CASES if c.N == 384} == {3}
    for rem in (4, 8, 12):
        assert any(c.tile and c.K % 16 == rem for c in T.CASES), f"K % 16 == {rem} on vector loads"
    assert any(c.tile and c.K < 16 for c in T.CASES)
    split = [c for c in T.CASES if c.nsplit > 1]
    assert any(c.bias_axis == 0 and c.alpha != 1 and c.ldc > c.N for c in split)
    assert any(c.bias_axis == 1 and c.alpha != 1 and c.Nc < c.N for c in split)
    assert any(c.stride_a == 0 and c.batch > 1 for c in T.CASES) and any(c.stride_b == 0 and c.batch > 1 for c in T.CASES)
    assert {c.tile for c in T.HARD_CASES} == {0, 1, 2, 3}
    assert {c.tile for c in T.HEAD_CASES} == {0, 1} and len(T.HEAD_CASES) == 18
    assert all(c.ldc > c.N and c.c_off for c in T.HEAD_CASES if c.name.startswith(("dq", "dk", "O =", "dV")))
    assert any(c.Kc == 24 and c.Kc < c.K for c in T.GROUP_CASES) and any(c.Nc == 16 and c.N == 48 for c in T.GROUP_CASES)


def test_every_launch_form_on_the_grid_has_a_case(grid_plans):
    have = {T.plan_key(c, pl) for c, pl in table_plans()}
    missing = [f"(layouts, tile, vec, split, ragged last split) = {k}, e.g. batch {v[0].batch} {v[0].M}x{v[0].N}x{v[0].K} "
               f"a_off {v[0].a_off}: {v[1]}" for k, v in sorted(grid_plans.items()) if k not in have and k not in UNREACHED]
    assert not missing, "launch forms without a case in tests/helpers/matmul_cases.py:\n" + "\n".join(missing)
    assert not set(UNREACHED) & have and set(UNREACHED) <= set(grid_plans), "UNREACHED is stale"
    # the grid is wide enough to see every layout pair on every tile in every split state
    want = {(lay, t, int(t != 0), s, r) for lay in T.LAYOUT.values() for t in range(4)
            for s, r in ((False, False), (True, False), (True, True))}
    assert set(grid_plans) == want, f"grid: missing {sorted(want - set(grid_plans))}, unexpected {sorted(set(grid_plans) - want)}"


def source_instances():
    """(A cols, B cols, WM, WN, MF, NF, vec) of every launch_mm named in dispatch_mm, for the four layout pairs that
    dispatch_layouts instantiates it with"""
    src = open(SRC).read()
    body = src[src.index("static void dispatch_mm("):]
    body = body[:body.index("\n}\n")]
    rows = re.findall(r"launch_mm<TileCfg<(\d+), (\d+), (\d+), (\d+)>, ACOL, BCOL, (true|false)>", body)
    assert len(rows) == 4 and body.count("launch_mm<") == 4, "dispatch_mm not understood"
    body = src[src.index("static void dispatch_layouts("):]
    body = body[:body.index("\n}\n")]
    pairs = re.findall(r"dispatch_mm<(true|false), (true|false)>", body)
    assert len(pairs) == 4 and len(set(pairs)) == 4 and body.count("dispatch_mm<") == 4, "dispatch_layouts not understood"
    # no launch of the kernel outside the two dispatch functions
    assert src.count("launch_mm<") == 4 and src.count("dispatch_mm<") == 4 and src.count("matmul_kernel<") == 1
    return {(int(a == "true"), int(b == "true"), int(wm), int(wn), int(mf), int(nf), int(vec == "true"))
            for a, b in pairs for wm, wn, mf, nf, vec in rows}


def test_every_kernel_instance_is_reached_by_a_case(grid_plans):
    inst = source_instances()
    assert len(inst) == 16
    got = {instance(*v) for v in grid_plans.values()}
    assert got <= inst, f"the plan query reports instances the source does not have: {sorted(got - inst)}"
    table = {}
    for c, pl in table_plans():
        table.setdefault(instance(c, pl), set()).add(pl["nsplit"] > 1)
    unreached = sorted(inst - set(table))
    assert not unreached, f"instances that no case reaches: {unreached}"
    one_state = sorted(k for k, v in table.items() if v != {False, True})
    assert not one_state, f"instances that run only with or only without split-K: {one_state}"


def test_workspace_agrees_with_the_plan():
    from buctd_amd import _C
    lib = _C.lib()
    for c in itertools.chain(T.CASES, grid()):
        pl = T.plan(c)
        d = T.desc(c)
        need = lib.buctd_matmul_workspace(C.byref(d))
        assert need == (c.batch * pl["nsplit"] * c.M * c.N * 4 if pl["nsplit"] > 1 else 0), f"{c}: {need} bytes, {pl}"


def test_the_builder_gives_every_case_small_disjoint_buffers():
    for c in T.CASES:
        b = T.build(c)            # asserts that no two elements of C, and of an operand that is not shared, coincide
        assert max(b.a_buf.numel(), b.b_buf.numel(), b.c_len) * 4 <= 4 << 20, T.case_id(c)
        assert b.A.shape == (c.batch, c.M, c.K) and b.B.shape == (c.batch, c.K, c.N) and b.c_addr.shape == (c.batch, c.M, c.N)
        a_addr, b_addr, _ = T.addresses(c)
        assert bool((b.a_buf[a_addr].double() == b.A).all()) and bool((b.b_buf[b_addr].double() == b.B).all()), T.case_id(c)
        assert int(torch.isfinite(b.a_buf).sum()) == a_addr.unique().numel(), T.case_id(c)
        assert int(torch.isfinite(b.b_buf).sum()) == b_addr.unique().numel(), T.case_id(c)
        assert c.M <= 400 and c.N <= 400 and c.K <= 2100


def test_query_and_launch_refuse_the_same_descriptors():
    from buctd_amd import _C
    lib = _C.lib()
    out = (C.c_int * len(T.PLAN_FIELDS))()
    good = T.mm("good", 2, 48, 48, 16, 0, 1, 1)
    assert T.plan(good) is not None
    # the pointers are never dereferenced: every call below returns before a launch
    ptrs = (T.BASE, T.BASE, None, T.BASE)
    bad = [good._replace(Kc=0), good._replace(Nc=0), good._replace(Kc=-4), good._replace(a_layout=2), good._replace(b_layout=2),
           good._replace(a_layout=-1), good._replace(M=0), good._replace(N=0), good._replace(K=0), good._replace(batch=0),
           good._replace(M=-3)]
    for c in bad:
        d = T.desc(c)
        assert lib.buctd_matmul_plan(C.byref(d), T.BASE, T.BASE, out) == EINVAL, c
        assert list(out) == [0] * len(T.PLAN_FIELDS)
        assert lib.buctd_matmul(C.byref(d), *ptrs, T.BASE, 1 << 30, None) == EINVAL, c
        assert b"buctd_matmul" in lib.buctd_last_error()
    d = T.desc(good)
    assert lib.buctd_matmul_plan(None, T.BASE, T.BASE, out) == EINVAL and lib.buctd_matmul_plan(C.byref(d), T.BASE, T.BASE, None) == EINVAL
    assert lib.buctd_matmul_plan(C.byref(d), None, T.BASE, out) == EINVAL and lib.buctd_matmul_plan(C.byref(d), T.BASE, None, out) == EINVAL
    assert lib.buctd_matmul(C.byref(d), T.BASE, T.BASE, None, None, None, 0, None) == EINVAL
    # a split plan without its workspace, or with one that is a float short
    for c in (c for c in T.CASES if c.nsplit > 1):
        d = T.desc(c)
        need = lib.buctd_matmul_workspace(C.byref(d))
        assert need > 0
        assert lib.buctd_matmul(C.byref(d), *ptrs, None, need, None) == EWORKSPACE, T.case_id(c)
        assert lib.buctd_matmul(C.byref(d), *ptrs, T.BASE, need - 4, None) == EWORKSPACE, T.case_id(c)
        assert lib.buctd_matmul(C.byref(d), *ptrs, T.BASE, 0, None) == EWORKSPACE, T.case_id(c)


def test_alignment_alone_moves_a_call_between_vector_and_scalar_loads():
    c = T.mm("aligned", 2, 48, 96, 16, 0, 1, 2)
    assert T.plan(c)["tile"] == 2 and T.plan(c._replace(a_off=4))["tile"] == 2
    for off in (1, 2, 3):
        assert T.plan(c._replace(a_off=off))["tile"] == 0 and T.plan(c._replace(b_off=off))["tile"] == 0
    assert T.plan(c, a_base=T.BASE + 8)["tile"] == 0 and T.plan(c, b_base=T.BASE + 4)["tile"] == 0
    # the split of K does not look at the loads (mm_split_plan counts tiles of the vector width either way)
    s = T.mm("split", 1, 48, 96, 1040, 0, 1, 2, 4)
    a, b = T.plan(s), T.plan(s._replace(b_off=1))
    assert (a["tile"], b["tile"]) == (2, 0) and (a["nsplit"], a["k_per_split"]) == (b["nsplit"], b["k_per_split"]) == (4, 272)
