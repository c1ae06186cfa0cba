"""Closure of the gathered bf16x6 case table (tests/helpers/gconv_cases.py) over the routes and plans of conv_gather_x6.hip and
conv_gather_wgrad.hip (host only: buctd_gconv_x6_plan / buctd_gconv_wgrad_x6_plan run the launch's own routing functions -
gc_geo, r1_ok, gc_plan, the epilogue choice; gw_plan - without a launch).

Every key that the routing can produce on the search grid must be reached by a case of the table, so a retuned threshold or a
new tile without a test shape fails here, by name; and every gc_launch / conv1x1_rows_x6_kernel / gw_launch instance in the two
sources is either reached or listed in UNREACHED with the reason."""
import itertools
import os
import re

import pytest

from tests.helpers import gconv_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "buctd_amd", "csrc")
TILES = {(4, 3, 2, 2): 96, (4, 4, 2, 2): 128, (2, 4, 4, 1): 64, (2, 3, 4, 1): 48}


def tile_of(pl):
    t = (pl["MF"], pl["NF"], pl["WM"], pl["WN"])
    assert pl["BM"] == t[2] * t[0] * 16 == 128 and pl["BN"] == t[3] * t[1] * 16 == TILES[t], pl
    return t


def tiled_key(case, pl):
    return (pl["BN"], case[0], case[1], pl["mode"])


def pipe_keys(pl):
    """per class (nsteps == 1, nsteps odd, nhs odd): what the step loop - unrolled by two, A pieces two steps ahead - sees"""
    return {(ns == 1, ns % 2 == 1, nhs % 2 == 1) for (_, nhs, ns) in pl["cls"]}


def rows_key(pl):
    return (pl["NFT"], pl["ksteps"] == 1)


def wgrad_key(case, pl):
    return (case[0], pl["CF"], pl["nsplit"] == 1, pl["rem"] == 0, pl["qrem"] == 0)


def sets_of(direction, rows=False):
    if rows:
        return T.ROWS_DGRAD_SETS if direction else T.ROWS_FWD_SETS
    return T.DGRAD_SETS if direction else T.FWD_SETS


@pytest.fixture(scope="module")
def grid_keys():
    """{key: first grid case} for the tiled kernel, its pipeline shapes, the row kernel and the weight gradient"""
    tiled, pipe, rows, wg = {}, {}, {}, {}
    flag_sets = {d: sorted(set(sets_of(d).values()) | set(sets_of(d, True).values())) for d in (T.FWD, T.DGRAD)}
    n = 0
    for kind, N, (H, W), Ci, Co in itertools.product(T.GRID_KINDS, T.GRID_N, T.GRID_HW, T.GRID_C, T.GRID_C):
        n += 1
        for d in (T.FWD, T.DGRAD):
            case = (kind, d, N, H, W, Ci, Co)
            for f in flag_sets[d]:
                pl = T.plan(case, f)
                if pl is None:
                    continue
                if pl["route"] == 1:
                    rows.setdefault(rows_key(pl), (case, f))
                else:
                    tiled.setdefault(tiled_key(case, pl), (case, f))
                    for k in pipe_keys(pl):
                        pipe.setdefault(k, (case, f))
        pl = T.wgrad_plan((kind, N, H, W, Ci, Co))
        if pl is not None:
            wg.setdefault(wgrad_key((kind,), pl), (kind, N, H, W, Ci, Co))
    assert n > 30000
    return tiled, pipe, rows, wg


def table_plans():
    """[(case, option set, flags, plan)] of every tiled and row case x option set of the table"""
    out = []
    for case, _ in T.TILED_CASES:
        out += [(case, name, f, T.plan(case, f)) for name, f in sets_of(case[1]).items()]
    for case, _, _ in T.ROW_CASES:
        out += [(case, name, f, T.plan(case, f)) for name, f in sets_of(case[1], True).items()]
    for case in T.HARD_CASES:
        out += [(case, name, f, T.plan(case, f)) for name, f in sets_of(case[1]).items()]
    return out


def test_every_case_takes_the_route_plan_and_mode_the_table_names():
    mode_of = {T.BIAS: -1, T.SCALE | T.RES | T.RELU: -1, 0: 0, T.ACC: T.C3M_STATS, T.PARTIALS: -1, T.RES: T.C3M_RES}
    for case, bn in T.TILED_CASES:
        for name, f in sets_of(case[1]).items():
            pl = T.plan(case, f)
            assert pl is not None and pl["route"] == 0, f"{case} {name}: {pl}"
            assert pl["BN"] == bn and TILES[tile_of(pl)] == bn and pl["mode"] == mode_of[f], f"{case} {name}: {pl}"
            assert T.positions(case) % pl["BM"] != 0, f"{case}: the last position tile is not ragged"
            assert pl["tiles"] == -(-T.positions(case) // pl["BM"]) and pl["ncol"] * bn == T.out_shape(case)[3]
            assert pl["ncls"] == (4 if case[:2] == (2, T.DGRAD) else 1)
            cpt = T.in_shape(case)[3] // 16
            taps = [1, 2, 2, 4] if pl["ncls"] == 4 else [1 if case[0] == 1 else 9]
            assert pl["cls"] == [(t, t * cpt, (t * cpt + 1) // 2) for t in taps], f"{case}: {pl}"
    # one case per (tile plan) x (kind, direction)
    assert {(bn, c[0], c[1]) for c, bn in T.PLAN_CASES} == set(itertools.product((96, 128, 64, 48), (1, 2), (0, 1)))
    assert len(T.PLAN_CASES) == 16
    for case, nft, ks in T.ROW_CASES:
        for name, f in sets_of(case[1], True).items():
            pl = T.plan(case, f)
            assert pl is not None and (pl["route"], pl["NFT"], pl["ksteps"]) == (1, nft, ks), f"{case} {name}: {pl}"
            assert nft * 16 == T.out_shape(case)[3] and ks * 32 == T.in_shape(case)[3]
        # an epilogue the row kernel lacks sends the same shape to the tiled kernel
        if case[1] == T.FWD:
            assert T.plan(case, T.PARTIALS)["route"] == 0 and T.plan(case, T.SCALE | T.RES | T.RELU)["route"] == 0
    for case, key, nsplit in T.WGRAD_CASES:
        pl = T.wgrad_plan(case)
        assert pl is not None and wgrad_key(case, pl) == key and pl["nsplit"] == nsplit, f"weight gradient {case}: {pl}"
        N, Ho, Wo = case[1], case[2] // (case[0]), case[3] // case[0]
        assert pl["ksteps"] == -(-N * Ho * Wo // 32) and pl["qrem"] == N * Ho * Wo % 32
        assert pl["nsplit"] * pl["q"] + pl["rem"] == pl["ksteps"] and (pl["TPG"], pl["ntg"]) == ((3, 3) if case[0] == 2 else (1, 1))
    for case in T.HARD_CASES:
        assert all(T.plan(case, f)["route"] == 0 for f in sets_of(case[1]).values())
    assert {c[:2] for c in T.HARD_CASES} == set(itertools.product((1, 2), (0, 1))) and {c[0] for c in T.WGRAD_HARD} == {1, 2}
    assert all(T.wgrad_plan(c) is not None for c in T.WGRAD_HARD)


def test_the_edges_the_table_promises():
    rows = lambda c: c[2] * c[3] * c[4]
    P = {c: T.plan(c, 0) for c, _ in T.TILED_CASES}
    cls = lambda kind, d: [(c, pl["cls"]) for c, pl in P.items() if c[:2] == (kind, d)]
    every = [k for c, pl in P.items() for k in pl["cls"]]
    assert any(ns == 1 and nhs == 1 for _, nhs, ns in every) and any(ns == 1 and nhs == 2 for _, nhs, ns in every)
    assert any(ns == 2 for _, nhs, ns in every) and any(ns >= 3 and ns % 2 for _, nhs, ns in every)
    # odd nhs = a dead last half-step: kind 1 with 16 and 48 source channels, kind 2 forward
    assert {T.in_shape(c)[3] for c, k in cls(1, T.FWD) + cls(1, T.DGRAD) if k[0][1] % 2} >= {16, 48}
    assert any(k[0][1] % 2 for c, k in cls(2, T.FWD)) and any(k[0][1] % 2 == 0 for c, k in cls(2, T.FWD))
    # stride-2 data gradient: class 0 (one tap) with a dead and with a live last half-step; classes 1-3 have 2, 2, 4 taps, so
    # their half-step count is even whatever the channels: they always end on a live one
    assert {k[0][1] % 2 for c, k in cls(2, T.DGRAD)} == {0, 1}
    assert all(nhs % 2 == 0 for c, k in cls(2, T.DGRAD) for _, nhs, _ in k[1:])
    assert any(c[3:5] == (2, 2) for c, _ in cls(2, T.FWD)) and any(c[3:5] == (2, 2) for c, _ in cls(2, T.DGRAD))
    assert any(c[3] == 2 and c[4] > 2 for c, _ in cls(2, T.FWD)) and any(c[4] == 2 and c[3] > 2 for c, _ in cls(2, T.FWD))
    assert any(c[3:5] == (1, 1) for c, _ in cls(1, T.FWD))
    # the 65535 / 65536-row boundary, and >= 65536 rows that stay on the tiled kernel
    assert any(rows(c) == 65535 and pl["route"] == 0 for c, pl in P.items())
    assert any(rows(c) >= 65536 and pl["BN"] == 128 for c, pl in P.items())
    for nft in (4, 8, 16):
        mine = [(c, ks) for c, n, ks in T.ROW_CASES if n == nft]
        assert any(ks == 1 for c, ks in mine) and any(ks > 1 for c, ks in mine), f"NFT {nft}: one and several K steps"
        biggest = max(ks for c, ks in mine)
        c = next(c for c, ks in mine if ks == biggest)
        more = list(c)
        more[6 if c[1] else 5] += 32
        assert T.plan(tuple(more), 0)["route"] == 0, f"NFT {nft}: {biggest} K steps is not the most r1_ok admits"
        assert any(rows(c) == 65536 for c, ks in mine) and any(rows(c) % 32 for c, ks in mine), f"NFT {nft}: exact and ragged rows"
    assert {c[1] for c, _, _ in T.ROW_CASES} == {T.FWD, T.DGRAD}
    wg = [(c, T.wgrad_plan(c)) for c, *_ in T.WGRAD_CASES]
    assert any(pl["CF"] == 4 and rows((0, 0) + c[1:]) == 65536 for c, pl in wg)
    assert any(pl["CF"] == 3 and c[4] % 32 == 0 and c[5] % 32 == 0 for c, pl in wg)
    assert any(c[3] // c[0] == 2 for c, pl in wg if c[0] == 1) and any(c[3] // c[0] == 2 for c, pl in wg if c[0] == 2)
    # guard cases: ragged, one per tile plan, row-kernel instance and CF
    assert {T.plan(c, 0)["BN"] for c in T.GUARD_TILED} == {96, 128, 64, 48} and all(T.positions(c) % 128 for c in T.GUARD_TILED)
    assert {T.plan(c, 0)["NFT"] for c in T.GUARD_ROWS} == {4, 8, 16} and all(rows(c) % 32 for c in T.GUARD_ROWS)
    assert {T.wgrad_plan(c)["CF"] for c in T.GUARD_WGRAD} == {2, 3, 4} and all(T.wgrad_plan(c)["qrem"] for c in T.GUARD_WGRAD)
    assert set(T.GUARD_TILED) <= {c for c, _ in T.TILED_CASES} and set(T.GUARD_ROWS) <= {c for c, _, _ in T.ROW_CASES}
    assert set(T.GUARD_WGRAD) <= {c for c, *_ in T.WGRAD_CASES} and set(T.PAD_CASES) <= {c for c, _ in T.TILED_CASES}
    assert all(T.plan(c, 0)["cls"][0][1] % 2 == 1 for c in T.PAD_CASES) and [c[:2] for c in T.PAD_CASES] == [(1, 0), (2, 0), (2, 1)]


def test_every_plan_on_the_grid_has_a_case(grid_keys):
    tiled, pipe, rows, wg = grid_keys
    have_t, have_p, have_r = set(), set(), set()
    for case, name, f, pl in table_plans():
        if pl["route"] == 1:
            have_r.add(rows_key(pl))
        else:
            have_t.add(tiled_key(case, pl))
            have_p.update(pipe_keys(pl))
    have_w = {wgrad_key(c, T.wgrad_plan(c)) for c, *_ in T.WGRAD_CASES}
    missing = [f"tiled (tile width, kind, dir, mode) = {k}, e.g. at {v[0]} with flags {v[1]}" for k, v in sorted(tiled.items())
               if k not in have_t]
    missing += [f"tiled pipeline (nsteps == 1, nsteps odd, nhs odd) = {k}, e.g. at {v[0]}" for k, v in sorted(pipe.items())
                if k not in have_p]
    missing += [f"rows (NFT, K steps == 1) = {k}, e.g. at {v[0]} with flags {v[1]}" for k, v in sorted(rows.items()) if k not in have_r]
    missing += [f"wgrad (kind, CF, nsplit == 1, rem == 0, Q % 32 == 0) = {k}, e.g. at {v}" for k, v in sorted(wg.items())
                if k not in have_w]
    assert not missing, "plans without a test shape in tests/helpers/gconv_cases.py:\n" + "\n".join(missing)
    # ... and the table names nothing the grid cannot see (a key that vanished: a threshold moved)
    gone = sorted(have_t - set(tiled)) + sorted(have_p - set(pipe)) + sorted(have_r - set(rows)) + sorted(have_w - set(wg))
    assert not gone, f"keys of the table that the search grid does not produce: {gone}"
    # the grid is wide enough to see every tile plan, row-kernel instance and CF
    assert {k[0] for k in tiled} == {96, 128, 64, 48} and {k[0] for k in rows} == {4, 8, 16} and {k[1] for k in wg} == {2, 3, 4}
    assert {(k[0], k[1], k[2]) for k in tiled} == set(itertools.product((96, 128, 64, 48), (1, 2), (0, 1)))


def source_instances():
    """("tiled", MF, NF, WM, WN, mode) from the gc_launch calls of gc_run x the kernel instances gc_launch names;
    ("rows", NFT); ("wgrad", CF, TPG)"""
    src = open(os.path.join(CSRC, "conv_gather_x6.hip")).read()
    inst = set()
    body = src[src.index("static int gc_launch("):]
    body = body[:body.index("\n}\n")]
    modes = re.findall(r"gconv_x6_kernel<MF, NF, WM, WN, ([\w-]+)>", body)
    assert sorted(modes) == ["-1", "0", "C3M_RES", "C3M_STATS"] and src.count("gconv_x6_kernel<") == 4, "gc_launch not understood"
    modes = [{"C3M_STATS": T.C3M_STATS, "C3M_RES": T.C3M_RES}.get(m) or int(m) for m in modes]
    tiles = re.findall(r"gc_launch<(\d+), (\d+), (\d+), (\d+)>\(", src)
    assert len(tiles) == 4 == len(set(tiles)) and src.count("gc_launch<") == 4, "gc_run not understood"
    for t in tiles:
        inst.update(("tiled",) + tuple(int(v) for v in t) + (m,) for m in modes)
    rows = re.findall(r"conv1x1_rows_x6_kernel<(\d+)>", src)
    assert len(rows) == 3 == len(set(rows))
    inst.update(("rows", int(v)) for v in rows)
    wsrc = open(os.path.join(CSRC, "conv_gather_wgrad.hip")).read()
    wg = re.findall(r"gw_launch<(\d+), (\d+)>\(", wsrc)
    assert len(wg) == 5 == len(set(wg)) and wsrc.count("gw_launch<") == 5
    inst.update(("wgrad", int(a), int(b)) for a, b in wg)
    return inst


# (instance, direction) pairs that no call reaches, and why.  The only place where something is left out.
UNREACHED = {}
for _t in TILES:
    UNREACHED[("tiled",) + _t + (-1, T.DGRAD)] = "the general epilogue on a data gradient: a data gradient carries no bias, scale, " \
        "relu or statistics, so only a tensor of 2 GB or more would take it - and gc_geo refuses those (32-bit byte offsets)"
    UNREACHED[("tiled",) + _t + (T.C3M_STATS, T.DGRAD)] = "no statistics on a data gradient (refused)"


def test_every_kernel_instance_is_reached_or_listed(grid_keys):
    tiled, pipe, rows, wg = grid_keys
    inst = source_instances()
    bn2tile = {v: k for k, v in TILES.items()}
    got = {("tiled",) + bn2tile[bn] + (mode,) for (bn, kind, d, mode) in tiled}
    got_dir = {("tiled",) + bn2tile[bn] + (mode, d) for (bn, kind, d, mode) in tiled}
    got |= {("rows", nft) for nft, _ in rows} | {("wgrad", cf, 3 if kind == 2 else 1) for (kind, cf, _, _, _) in wg}
    assert got <= inst, f"the plan queries report instances the source does not have: {sorted(got - inst)}"
    assert not sorted(inst - got), f"instances that no grid shape reaches: {sorted(inst - got)}"
    # per direction: every (instance, direction) is reached or explained
    want_dir = {i + (d,) for i in inst if i[0] == "tiled" for d in (T.FWD, T.DGRAD)}
    unlisted = sorted(want_dir - got_dir - set(UNREACHED))
    assert not unlisted, f"(instance, direction) that no grid shape reaches and UNREACHED does not explain: {unlisted}"
    assert not set(UNREACHED) & got_dir and set(UNREACHED) <= want_dir, "UNREACHED is stale"
    # ... and the table reaches every one the grid reaches
    table = set()
    for case, name, f, pl in table_plans():
        table.add(("rows", pl["NFT"]) if pl["route"] else ("tiled",) + tile_of(pl) + (pl["mode"], case[1]))
    table |= {("wgrad", T.wgrad_plan(c)["CF"], 3 if c[0] == 2 else 1) for c, *_ in T.WGRAD_CASES}
    reach = got_dir | {i for i in got if i[0] != "tiled"}
    assert reach <= table, f"reached on the grid but by no case: {sorted(reach - table)}"


def test_plan_query_refuses_what_the_launch_refuses_and_agrees_with_its_siblings():
    import ctypes as C
    from buctd_amd import _C
    lib = _C.lib()
    ok = (1, T.FWD, 2, 8, 6, 48, 48)
    assert T.plan(ok, 0) is not None
    assert T.plan((3, T.FWD, 2, 8, 6, 48, 48)) is None and T.plan((1, T.FWD, 2, 8, 6, 40, 48)) is None     # kind, Ci % 16
    assert T.plan((2, T.FWD, 2, 9, 6, 48, 48)) is None and T.plan((1, T.FWD, 2, 8, 6, 48, 32)) is None     # odd H, 32 outputs
    assert T.plan((1, 2, 2, 8, 6, 48, 48)) is None and T.plan(ok, 64) is None and T.plan(ok, -1) is None
    assert T.plan((1, T.DGRAD, 2, 8, 6, 48, 48), T.BIAS) is None and T.plan((1, T.DGRAD, 2, 8, 6, 48, 48), T.ACC) is None
    assert T.plan(ok, T.ACC | T.RES) is None and T.plan(ok, T.ACC | T.BIAS)["mode"] == -1
    assert lib.buctd_gconv_x6_plan(*ok, 0, None) != 0
    assert T.wgrad_plan((1, 2, 8, 1, 48, 48)) is None and T.wgrad_plan((1, 2, 8, 6, 48, 16)) is None     # Wo < 2, no chunk pair
    assert T.wgrad_plan((2, 2, 9, 8, 48, 48)) is None and lib.buctd_gconv_wgrad_x6_plan(1, 2, 8, 6, 48, 48, None) != 0
    for case, *_ in T.TILED_CASES + T.ROW_CASES:
        kind, d, N, H, W, Ci, Co = case
        assert lib.buctd_gconv_x6_supported(kind, N, H, W, Ci, Co, d) == 1
        if d == T.FWD:      # the row groups of the partial-sum statistics come from the same plan
            ng, rpg = C.c_int(), C.c_int()
            pl = T.plan(case, T.PARTIALS)
            assert lib.buctd_gconv_x6_stats_groups(kind, N, H, W, Ci, Co, C.byref(ng), C.byref(rpg)) == 0
            assert rpg.value == pl["MF"] * 16 and ng.value == pl["tiles"] * pl["WM"], case
    for case, *_ in T.WGRAD_CASES:
        pl = T.wgrad_plan(case)
        assert lib.buctd_gconv_wgrad_x6_supported(*case) == 1
        pairs = (case[4] // (pl["CF"] * 16)) * (case[5] // (pl["CF"] * 16))
        assert lib.buctd_gconv_wgrad_x6_workspace(*case) == pairs * pl["ntg"] * pl["nsplit"] * pl["TPG"] * pl["CF"] ** 2 * 1024


def test_signatures_and_header_agree_on_the_plan_queries():
    from buctd_amd import _C
    hdr = open(os.path.join(ROOT, "include", "buctd_hip.h")).read()
    for name, nint in (("buctd_gconv_x6_plan", 8), ("buctd_gconv_wgrad_x6_plan", 6)):
        m = re.search(r"\bint %s\(([^)]*)\);" % name, hdr)
        assert m, f"{name} is not declared in include/buctd_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nint + 1 and all(a.startswith("int ") for a in args[:-1]) and args[-1] == "int* out"
        res, argtypes = _C.SIGNATURES[name]
        assert len(argtypes) == nint + 1
