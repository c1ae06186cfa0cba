"""Closure of the thin-channel convolution case table (tests/helpers/conv_thin_cases.py) over the thin routes of conv.hip
(host only: buctd_conv2d_plan runs the routing functions of buctd_conv2d_fwd / _dgrad / _wgrad without a launch).

Every (direction, route, instance key) that fwd_route / dgrad_route / wgrad_route and the helper's key() produce on the search
grid - the model's own 384x288 and 256x192 at N = 32 included, whose tile and row loops run 13 and 12 times - must be the key
of a table case, and no two cases share a key: a retuned threshold, a new instance, or a case taken out of the table fails
here, by name.  The helper's tile and segment arithmetic is tied to the library's through nsplit and the workspace size, its
constants to the source text."""
import ctypes as C
import itertools
import os
import re

import pytest

from tests.helpers import conv_thin_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "buctd_amd", "csrc", "conv.hip")
DIRS = {T.FWD: "forward", T.DGRAD: "data gradient", T.WGRAD: "weight gradient"}
THIN_ROUTES = {T.FWD: {1, 2, 3, 4}, T.DGRAD: {1, 2, 3, 4}, T.WGRAD: {1, 2, 3}}


def grid():
    return itertools.product(T.GRID_N, T.GRID_HW, T.GRID_C, T.GRID_C, T.GRID_GEO)


def flag_sets(direction):
    return (0, T.STATS) if direction == T.FWD else (0,)      # statistics are part of the thin-input forward key


@pytest.fixture(scope="module")
def grid_keys():
    """{(direction, route, key): first grid shape} over the thin routes of the grid"""
    found, n = {}, 0
    for N, (H, W), Ci, Co, (k, s, p) in grid():
        case = (N, H, W, Ci, Co, k, s, p)
        n += 1
        for direction in DIRS:
            for flags in flag_sets(direction):
                pl = T.plan(case, direction, flags)
                assert pl is not None, (case, direction, flags)
                if pl["route"]:
                    found.setdefault((direction, pl["route"], T.key(case, direction, pl["route"], flags)), case)
    assert n > 40000
    return found


def table():
    """[(direction, case, flags, route the table names, nsplit or None)]"""
    rows = []
    for case, route in T.FWD_CASES:
        rows += [(T.FWD, case, f, route, None) for f in ((0, T.STATS) if route == 4 else (0,))]
    rows += [(T.DGRAD, case, 0, route, None) for case, route in T.DGRAD_CASES]
    rows += [(T.WGRAD, case, 0, route, ns) for case, route, ns in T.WGRAD_CASES]
    return rows


def table_keys():
    return [(d, route, T.key(case, d, route, flags)) for d, case, flags, route, ns in table()]


def test_every_case_reports_the_route_and_nsplit_the_table_names():
    for direction, case, flags, route, ns in table():
        pl = T.plan(case, direction, flags)
        assert pl is not None and pl["route"] == route and route in THIN_ROUTES[direction], \
            f"{DIRS[direction]} {case} flags {flags}: the table names route {route}, the plan query reports {pl}"
        assert T.tensor_floats(case) <= T.MAX_FLOATS, f"{case}: a tensor of {T.tensor_floats(case)} floats"
        if direction == T.WGRAD:
            assert pl["nsplit"] == ns == T.nsplit_of(case, route), \
                f"weight gradient {case}: nsplit {pl['nsplit']} (library), {ns} (table), {T.nsplit_of(case, route)} (helper)"
        # bias is not part of the routing of a thin forward
        if direction == T.FWD:
            assert T.plan(case, direction, flags | T.BIAS)["route"] == route


def test_no_two_cases_share_a_key():
    keys = table_keys()
    twice = sorted({k for k in keys if keys.count(k) > 1})
    assert not twice, f"cases of tests/helpers/conv_thin_cases.py with the same key (one of each is redundant): {twice}"


def test_every_key_on_the_grid_has_a_case(grid_keys):
    have = set(table_keys())
    missing = [f"{DIRS[d]} route {r} ({T.ROUTE_NAMES[(d, r)]}): {' / '.join(k)}, e.g. at {grid_keys[(d, r, k)]}"
               for d, r, k in sorted(grid_keys) if (d, r, k) not in have]
    assert not missing, "keys without a case in tests/helpers/conv_thin_cases.py:\n" + "\n".join(missing)
    # the only cases beyond the grid (whose channels end at 64): Co = 256, the largest filter image of the stride-2 data
    # gradient, once per parity of (H, W)
    beyond = {(T.DGRAD, 1, (f"Ci={ci}", "Co=256", f"H%2={h}", f"W%2={w}")) for ci, h, w in ((3, 0, 0), (1, 0, 1), (4, 1, 0), (2, 1, 1))}
    assert have - set(grid_keys) == beyond, f"cases whose key the grid does not reach: {sorted(have - set(grid_keys) - beyond)}"
    # the grid is wide enough to see every thin route, every template instance and both sides of both loop caps
    assert {(d, r) for d, r, k in grid_keys} == {(d, r) for d in THIN_ROUTES for r in THIN_ROUTES[d]}
    assert {k[0] for d, r, k in grid_keys if (d, r) == (T.WGRAD, 2)} == {"<7,true>", "<7,false>", "<3,false>"}
    assert {k[2] for d, r, k in grid_keys if (d, r) == (T.WGRAD, 2)} == {"one pass", "loop"}
    assert {k[:2] for d, r, k in grid_keys if (d, r) == (T.WGRAD, 3)} == {(f"CI={c}", f"ST={s}") for c in (1, 2, 3, 4) for s in (1, 2)}
    assert {k[:2] for d, r, k in grid_keys if (d, r) == (T.FWD, 4)} == {(f"CI={c}", f"ST={s}") for c in (1, 2, 3, 4) for s in (1, 2)}


def test_the_models_own_shapes_are_on_the_grid_and_loop():
    assert {32} <= set(T.GRID_N) and {(384, 288), (256, 192)} <= set(T.GRID_HW)
    have = set(table_keys())
    for hw, loops in (((384, 288), (13824, 12288)), ((256, 192), (6144, 8192))):
        out3, both, in3, stem = (32, *hw, 64, 3, 7, 1, 3), (32, *hw, 3, 3, 7, 1, 3), (32, *hw, 3, 64, 3, 1, 1), (32, *hw, 3, 64, 3, 2, 1)
        assert T.wgrad_tiles(both) == loops[0] and 32 * hw[0] == loops[1]
        for direction, case, route in ((T.FWD, out3, 2), (T.FWD, both, 1), (T.FWD, in3, 4), (T.FWD, stem, 4),
                                       (T.DGRAD, out3, 3), (T.DGRAD, both, 2), (T.DGRAD, stem, 1),
                                       (T.WGRAD, out3, 1), (T.WGRAD, both, 2), (T.WGRAD, in3, 3), (T.WGRAD, stem, 3)):
            assert T.plan(case, direction)["route"] == route, (direction, case)
            assert (direction, route, T.key(case, direction, route)) in have, (direction, case)
        assert T.key(both, T.WGRAD, 2)[-1] == "loop" and T.key(in3, T.WGRAD, 3)[-1] == "loop"
    # the loop cases of the table: more items than workgroups and no multiple of them, so workgroups take different counts
    for case, route, ns in T.WGRAD_CASES:
        if T.is_loop_case(case, route):
            items = T.wgrad_tiles(case) if route == 2 else case[0] * T.out_hw(case)[0]
            assert ns == 1024 < items < 2048 and items % 1024, (case, items)
            half = (case[0] // 2,) + case[1:]       # half the batch stays below the cap: the GPU test's two-call reference
            hpl = T.plan(half, T.WGRAD)
            assert hpl["route"] == route and hpl["nsplit"] < 1024, (half, hpl)


def test_tile_constants_equal_the_source():
    src = open(SRC).read()
    consts = {}
    for line in re.findall(r"^constexpr int ([^;]+);", src, re.M):
        for name, value in re.findall(r"(\w+) = (\d+)", line):
            consts[name] = int(value)
    for name in T.CONSTANTS:
        assert consts.get(name) == getattr(T, name), f"{name}: {getattr(T, name)} in the helper, {consts.get(name)} in conv.hip"
    # the instances the keys name are the instances the source launches
    assert set(re.findall(r"conv_wgrad_thin_kernel<(\d), (true|false)>\)", src)) == {("7", "true"), ("7", "false"), ("3", "false")}
    assert set(re.findall(r"conv_fwd_thin_px4_kernel<7, (\d), CH, TR>", src)) == {"1", "2", "3"}
    assert set(re.findall(r"launch_thin_px4<(\d), (true|false)>", src)) == {("4", "false"), ("8", "false"), ("4", "true")}
    assert src.count("THIN_IN_FWD(1) THIN_IN_FWD(2) THIN_IN_FWD(3) THIN_IN_FWD(4)") == 1
    assert src.count("THIN_IN_WG(1) THIN_IN_WG(2) THIN_IN_WG(3) THIN_IN_WG(4)") == 1


def test_threshold_pairs():
    for direction, inside, r_in, outside, r_out, line in T.THRESHOLDS:
        pi, po = T.plan(inside, direction), T.plan(outside, direction)
        assert pi is not None and pi["route"] == r_in, f"{line}: {DIRS[direction]} {inside} reports {pi}, not route {r_in}"
        assert po is not None and po["route"] == r_out, f"{line}: {DIRS[direction]} {outside} reports {po}, not route {r_out}"
    lines = " ".join(t[5] for t in T.THRESHOLDS)
    for predicate in ("fwd_thin_ok", "dgrad_thin_s2_ok", "fwd_thin_in_ok", "wgrad_thin_ok", "wgrad_thin_rows_ok"):
        assert predicate in lines
        assert re.search(rf"static bool {predicate}\(", open(SRC).read())


def test_flags_that_leave_the_thin_routes():
    for direction, case, route, flags, route_with in T.FLAG_CASES:
        assert T.plan(case, direction, 0)["route"] == route, (direction, case)
        pl = T.plan(case, direction, flags)
        assert pl is not None and pl["route"] == route_with, f"{DIRS[direction]} {case} flags {flags}: {pl}, not route {route_with}"
    for direction, case, flags in T.REFUSED:
        assert T.plan(case, direction, 0)["route"] == 4
        assert T.plan(case, direction, flags) is None, f"{case} flags {flags}: statistics with an epilogue must be refused"


def test_workspace_is_nsplit_slabs():
    from buctd_amd import _C
    lib = _C.lib()
    for case, route, ns in T.WGRAD_CASES:
        N, H, W, Ci, Co, k, s, p = case
        d = T.desc(case)
        assert lib.buctd_conv2d_wgrad_workspace(C.byref(d)) == ns * Co * k * k * Ci * 4, case


def test_guard_and_hard_cases_are_table_cases_one_per_route_and_kernel():
    rows = {(d, case, route) for d, case, flags, route, ns in table()}
    for entry in T.GUARD_CASES + T.HARD_CASES:
        assert entry in rows, f"{entry} is not a case of the table"
    assert len(T.GUARD_CASES) == 12 and {(d, r) for d, c, r in T.GUARD_CASES} == {(d, r) for d in THIN_ROUTES for r in THIN_ROUTES[d]}
    assert len(T.HARD_CASES) == 9 and {(d, r) for d, c, r in T.HARD_CASES} == {(d, r) for d in (T.FWD, T.DGRAD) for r in (1, 2, 3, 4)}
