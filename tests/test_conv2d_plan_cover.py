"""Closure of the exact-fp32 convolution case table (tests/helpers/conv2d_cases.py) over the implicit-GEMM plans of conv.hip
(host only: buctd_conv2d_plan runs the routing functions of buctd_conv2d_fwd / _dgrad / _wgrad without a launch).

Every implicit-GEMM plan that fwd_route / dgrad_route / wgrad_route can pick on the search grid must be reached by a case of the
table - so a retuned threshold or a new tile without a test shape fails here, by name - and every launch_conv / launch_wgrad
instance in the source is either reached or listed in UNREACHED with the reason."""
import ctypes as C
import itertools
import os
import re

import pytest

from tests.helpers import conv2d_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "buctd_amd", "csrc", "conv.hip")

# implicit-GEMM instances that no grid shape reaches, and why.  The only place where instances are left out.
UNREACHED = {}


def conv_key(pl):
    return (pl["tile"], pl["vec"], pl["par"])


def wgrad_key(case, pl):
    """(configuration, nsplit == 1, last split ragged, float4 slab reduction)"""
    return (pl["tile"], pl["nsplit"] == 1, T.rows_of(case, T.WGRAD) % pl["pix_per_split"] != 0, pl["vec_reduce"] == 1)


def instance(direction, pl):
    """the template instance a plan launches: (direction, WM, WN, MF, NF, vec)"""
    wn = 4 // pl["WM"]
    assert pl["BM"] == pl["WM"] * pl["MF"] * 16 and pl["BN"] % (wn * 16) == 0, pl
    return (direction, pl["WM"], wn, pl["MF"], pl["BN"] // (wn * 16), pl["vec"])


def grid():
    for N, (H, W), Ci, Co, (k, s, p) in itertools.product(T.GRID_N, T.GRID_HW, T.GRID_C, T.GRID_C, T.GRID_GEO):
        if H + 2 * p >= k and W + 2 * p >= k:
            yield (N, H, W, Ci, Co, k, s, p)


@pytest.fixture(scope="module")
def grid_plans():
    """{direction: {key: (first grid shape, flags, plan)}} over the implicit-GEMM plans of the grid"""
    found = {T.FWD: {}, T.DGRAD: {}, T.WGRAD: {}}
    n = 0
    for case in grid():
        n += 1
        for direction, flag_sets in ((T.FWD, T.FWD_FLAGS), (T.DGRAD, T.DGRAD_FLAGS)):
            for flags in flag_sets.values():
                pl = T.plan(case, direction, flags)
                if pl is not None and pl["route"] == 0:
                    found[direction].setdefault(conv_key(pl), (case, flags, pl))
        pl = T.plan(case, T.WGRAD)
        assert pl is not None, case
        if pl["route"] == 0:
            found[T.WGRAD].setdefault(wgrad_key(case, pl), (case, 0, pl))
    assert n > 50000
    return found


def table_plans():
    """[(direction, case, flags, plan)] of every case x option set of the table"""
    rows = []
    for case, tile in T.FWD_CASES + [T.HARD_CASE]:
        rows += [(T.FWD, case, f, T.plan(case, T.FWD, f)) for f in T.FWD_FLAGS.values()]
    for case, tile, par in T.DGRAD_CASES + [T.HARD_CASE + (0,)]:
        rows += [(T.DGRAD, case, f, T.plan(case, T.DGRAD, f)) for f in T.DGRAD_FLAGS.values()]
    rows += [(T.WGRAD, case, 0, T.plan(case, T.WGRAD)) for case, cfg, ns in T.WGRAD_CASES]
    return rows


def test_every_case_is_on_the_implicit_gemm_route_with_the_plan_the_table_names():
    for direction, case, flags, pl in table_plans():
        assert pl is not None and pl["route"] == 0, f"direction {direction} {case} flags {flags}: {pl}"
    for case, tile in T.FWD_CASES:
        for f in T.FWD_FLAGS.values():
            pl = T.plan(case, T.FWD, f)
            assert (pl["tile"], pl["par"]) == (tile, 0), f"forward {case} flags {f}: {pl}"
    for case, tile, par in T.DGRAD_CASES:
        pl = T.plan(case, T.DGRAD, 0)
        assert (pl["tile"], pl["par"]) == (tile, par), f"data gradient {case}: {pl}"
        assert T.plan(case, T.DGRAD, T.BIAS | T.STATS)["tile"] == tile
    for case, cfg, ns in T.WGRAD_CASES:
        pl = T.plan(case, T.WGRAD)
        assert (pl["tile"], pl["nsplit"]) == (cfg, ns), f"weight gradient {case}: {pl}"
    # statistics switch the parity split off: their row groups are rows of the whole gradient
    assert T.plan(T.DGRAD_STATS_PAR0, T.DGRAD, 0)["par"] == 1 and T.plan(T.DGRAD_STATS_PAR0, T.DGRAD, T.BIAS | T.STATS)["par"] == 0
    for c in (T.GUARD_FWD, T.GUARD_DGRAD, T.GUARD_WGRAD):
        assert c in [r[1] for r in table_plans()]
    assert T.plan(T.GUARD_FWD, T.FWD, T.BIAS)["vec"] == 0 and T.plan(T.GUARD_DGRAD, T.DGRAD)["par"] == 1
    assert T.plan(T.GUARD_WGRAD, T.WGRAD)["nsplit"] > 1


def test_every_plan_on_the_grid_has_a_case(grid_plans):
    have = {T.FWD: set(), T.DGRAD: set(), T.WGRAD: set()}
    for direction, case, flags, pl in table_plans():
        have[direction].add(wgrad_key(case, pl) if direction == T.WGRAD else conv_key(pl))
    names = {T.FWD: "forward (tile, vec, par)", T.DGRAD: "data gradient (tile, vec, par)",
             T.WGRAD: "weight gradient (configuration, nsplit == 1, last split ragged, float4 reduction)"}
    missing = [f"{names[d]} = {k}, e.g. at {v[0]} with flags {v[1]}"
               for d in grid_plans for k, v in sorted(grid_plans[d].items()) if k not in have[d]]
    assert not missing, "plans without a test shape in tests/helpers/conv2d_cases.py:\n" + "\n".join(missing)
    # the grid is wide enough to see every tile id and every weight-gradient configuration
    assert {k[0] for k in grid_plans[T.FWD]} == set(range(11)) and {k[0] for k in grid_plans[T.DGRAD]} == set(range(11))
    assert {k for k in grid_plans[T.DGRAD] if k[2]} == {(t, 1, 1) for t in range(1, 11)}
    assert {k[0] for k in grid_plans[T.WGRAD]} == set(range(5))


def source_instances():
    """(direction, WM, WN, MF, NF, vec) of every launch_conv named in dispatch_conv (both directions) and every launch_wgrad
    named in dispatch_wgrad"""
    src = open(SRC).read()
    inst = set()
    body = src[src.index("static void dispatch_conv("):]
    body = body[:body.index("\n}\n")]
    rows = re.findall(r"launch_conv<TileCfg<(\d+), (\d+), (\d+), (\d+)>, DGRAD, (true|false)>", body)
    assert len(rows) == 11 and body.count("launch_conv<") == 11, "dispatch_conv not understood"
    for wm, wn, mf, nf, vec in rows:
        for direction in (T.FWD, T.DGRAD):
            inst.add((direction, int(wm), int(wn), int(mf), int(nf), int(vec == "true")))
    body = src[src.index("static void dispatch_wgrad("):]
    body = body[:body.index("\n}\n")]
    rows = re.findall(r"launch_wgrad<TileCfg<(\d+), (\d+), (\d+), (\d+)>, (true|false)>", body)
    assert len(rows) == 5 and body.count("launch_wgrad<") == 5, "dispatch_wgrad not understood"
    for wm, wn, mf, nf, vec in rows:
        inst.add((T.WGRAD, int(wm), int(wn), int(mf), int(nf), int(vec == "true")))
    # no launch of these kernels outside the two dispatch functions
    assert src.count("launch_conv<") == 11 and src.count("launch_wgrad<") == 5
    assert src.count("conv_gemm_kernel<") == 1 and src.count("conv_wgrad_kernel<") == 1
    return inst


def test_every_kernel_instance_is_reached_or_listed(grid_plans):
    inst = source_instances()
    got = {instance(d, v[2]) for d in grid_plans for v in grid_plans[d].values()}
    assert got <= inst, f"the plan query reports instances the source does not have: {sorted(got - inst)}"
    unlisted = sorted(inst - got - set(UNREACHED))
    assert not unlisted, f"instances that no grid shape reaches and UNREACHED does not explain: {unlisted}"
    assert not set(UNREACHED) & got and set(UNREACHED) <= inst, "UNREACHED is stale"
    table = {instance(d, pl) for d, case, flags, pl in table_plans()}
    assert got <= table, f"reached on the grid but by no case: {sorted(got - table)}"
    # the dead thin weight-gradient instance (3x3 with the wide side on dy, which wgrad_thin_ok refuses) stays out
    assert "conv_wgrad_thin_kernel<3, true>" not in open(SRC).read()


def test_query_agrees_with_stats_groups_and_workspace():
    from buctd_amd import _C
    lib = _C.lib()
    for direction, case, flags, pl in table_plans():
        d = T.desc(case)
        if direction == T.WGRAD:
            N, H, W, Ci, Co, k, s, p = case
            assert lib.buctd_conv2d_wgrad_workspace(C.byref(d)) == pl["nsplit"] * Co * k * k * Ci * 4, case
            M = T.rows_of(case, T.WGRAD)
            assert pl["pix_per_split"] % 16 == 0 and (pl["nsplit"] - 1) * pl["pix_per_split"] < M <= pl["nsplit"] * pl["pix_per_split"]
            assert pl["vec_reduce"] == int((Co * k * k * Ci) % 4 == 0) and pl["BN"] == 64
            continue
        ng, rpg = C.c_int(), C.c_int()
        assert lib.buctd_conv2d_stats_groups(C.byref(d), direction, C.byref(ng), C.byref(rpg)) == 0
        M = T.rows_of(case, direction)
        assert rpg.value == pl["MF"] * 16 and ng.value == -(-M // pl["BM"]) * pl["WM"], f"direction {direction} {case}: {pl}"


def test_query_refuses_what_the_launch_refuses_and_names_the_thin_routes():
    from buctd_amd import _C
    lib = _C.lib()
    out = (C.c_int * len(T.PLAN_FIELDS))()
    d = T.desc((2, 9, 7, 20, 30, 3, 1, 1))
    assert lib.buctd_conv2d_plan(C.byref(d), 3, 0, out) != 0 and lib.buctd_conv2d_plan(C.byref(d), 0, 32, out) != 0
    assert lib.buctd_conv2d_plan(C.byref(d), 1, T.RELU, out) != 0 and lib.buctd_conv2d_plan(C.byref(d), 2, T.BIAS, out) != 0
    assert lib.buctd_conv2d_plan(C.byref(d), 0, 0, None) != 0 and lib.buctd_conv2d_plan(None, 0, 0, out) != 0
    bad = T.desc((2, 9, 7, 20, 30, 3, 1, 1))
    bad.Ho += 1
    assert lib.buctd_conv2d_plan(C.byref(bad), 0, 0, out) != 0
    # the preNet shapes of test_gpu_conv_thin.py leave route 0 - and come back to it with an epilogue the thin kernels lack
    thin_out, thin_both, thin_in = (2, 192, 256, 64, 3, 7, 1, 3), (3, 160, 144, 3, 3, 7, 1, 3), (2, 192, 256, 3, 64, 3, 1, 1)
    assert T.plan(thin_out, T.FWD, T.BIAS)["route"] == 2 and T.plan(thin_both, T.FWD, T.BIAS)["route"] == 1
    assert T.plan((2, 181, 203, 17, 4, 7, 1, 3), T.FWD)["route"] == 3 and T.plan(thin_in, T.FWD, T.BIAS | T.STATS)["route"] == 4
    assert T.plan(thin_out, T.FWD, T.BIAS | T.RELU)["route"] == 0 and T.plan(thin_out, T.FWD, T.STATS)["route"] == 0
    assert T.plan(thin_in, T.FWD, T.RELU)["route"] == 0 and T.plan(thin_in, T.FWD, T.STATS | T.RELU) is None
    assert T.plan((2, 192, 256, 3, 64, 3, 2, 1), T.DGRAD)["route"] == 1 and T.plan(thin_both, T.DGRAD)["route"] == 2
    assert T.plan(thin_out, T.DGRAD)["route"] == 3 and T.plan((2, 181, 203, 17, 4, 7, 1, 3), T.DGRAD)["route"] == 4
    assert T.plan(thin_out, T.DGRAD, T.BIAS)["route"] == 0
    assert T.plan(thin_out, T.WGRAD)["route"] == 1 and T.plan(thin_both, T.WGRAD)["route"] == 2
    assert T.plan(thin_in, T.WGRAD)["route"] == 3 and T.plan((2, 181, 203, 4, 48, 3, 1, 1), T.WGRAD)["route"] == 0
    for case in (thin_out, thin_both, thin_in):
        d = T.desc(case)
        N, H, W, Ci, Co, k, s, p = case
        assert lib.buctd_conv2d_wgrad_workspace(C.byref(d)) == T.plan(case, T.WGRAD)["nsplit"] * Co * k * k * Ci * 4
