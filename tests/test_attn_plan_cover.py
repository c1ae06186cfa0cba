"""Closure of the narrow-contraction attention case table (tests/helpers/attn_cases.py) over the routing of attn_smallqk.hip
(host only: buctd_attn_smallqk_plan runs attn_route, the routing function of the launches, without a launch).

Every route the query can report on the supported grid must be reached by a case of the table - so a new C / R4 instance or a
changed routing rule without a test case fails here, by name - and every attn_launch<R4, CF> the source's dispatch names is
reached in each of its kernel families.  The input families are checked on the fp64 reference alone: a case that claims a
moving maximum has one."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

from tests.helpers import attn_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "buctd_amd", "csrc", "attn_smallqk.hip")

# routes that a caller could expect and the routing never reports, and why: (family, R4, CF, pieces).  The only place where
# routes are left out.
UNREACHED = {
    (1, 4, 12, 3): "attn_split_mode: three pieces at C = 192 would need 77 KB of static LDS, the width stays on the fp32 kernels",
    (1, 8, 12, 3): "attn_split_mode: three pieces at C = 192 would need 77 KB of static LDS, the width stays on the fp32 kernels",
}

EINVAL = -1
BASE = 1 << 20          # a pointer value that is never dereferenced


def grid():
    for t, r4, c, flag, p, dseed in itertools.product(T.TS, T.R4S, T.CS, T.FLAGS, (0.0, T.P_DROP), (False, True)):
        yield t, r4, c, flag, p, dseed


def drop_dseed(key):
    """a route without its seed form: the table holds value-seed cases, the GPU test runs the device-seed form of every
    (R4, C, flag) with dropout beside them (test_device_seed_form_is_bit_equal)"""
    return key[:6]


@pytest.fixture(scope="module")
def grid_routes():
    found = {}
    n = 0
    for args in grid():
        n += 1
        pl = T.plan(*args)
        assert pl is not None, args
        found.setdefault(T.route_key(pl), args)
    assert n == 3 * 4 * 7 * 3 * 2 * 2
    return found


def test_the_table_is_the_one_the_issue_sets():
    ids = [T.case_id(c) for c in T.CASES]
    assert len(set(ids)) == len(ids), "case ids repeat"
    full = {(c.R4, c.C, c.flag, c.p) for c in T.CASES if c.T == 128}
    assert full == set(itertools.product(T.R4S, T.CS, T.FLAGS, (0.0, T.P_DROP))) and len(full) == 28 * 3 * 2
    assert sorted((c.R4, c.C, c.flag) for c in T.CASES if c.T == 64) == sorted(itertools.product(T.R4S, T.CS, T.FLAGS))
    assert sorted((c.R4, c.flag) for c in T.CASES if c.T == 576) == sorted(itertools.product(T.R4S, T.FLAGS))
    assert {c.T for c in T.CASES} == set(T.TS) and T.B == 2
    assert T.SEED >> 32 != T.SEED & 0xFFFFFFFF and T.P_DROP == 0.3
    assert {c.p for c in T.CASES} == {0.0, 0.3}
    for c in T.CASES:
        assert T.route(c) is not None, f"{T.case_id(c)}: the launch would refuse the case"


def test_the_query_states_the_routing_rules(grid_routes):
    """what the header promises, read off the query: wide contractions and three pieces at C = 192 take the fp32 kernels, the
    split forward needs no statistics pass, the device seed is read by dropout kernels only"""
    for t, r4, c, flag, p, dseed in grid():
        pl = T.plan(t, r4, c, flag, p, dseed)
        pieces = 0 if r4 > 8 or flag == 0 or (flag == 2 and c == 192) else (3 if flag == 2 else 2)
        want = dict(split=int(pieces != 0), R4=r4, CF=c // 16, pieces=pieces, stats=int(pieces == 0), drop=int(p > 0),
                    dseed=int(p > 0 and dseed))
        assert pl == want, ((t, r4, c, flag, p, dseed), pl)
    assert len(grid_routes) == (28 + 14 + 12) * 3      # fp32, two pieces, three pieces x {no dropout, value seed, device seed}


def test_every_route_on_the_grid_has_a_case(grid_routes):
    have = {drop_dseed(T.route_key(T.route(c))) for c in T.CASES}
    missing = [f"(family, R4, CF, pieces, stats, drop) = {drop_dseed(k)}, e.g. (T, R4, C, flag, p, dseed) = {v}"
               for k, v in sorted(grid_routes.items()) if drop_dseed(k) not in have]
    assert not missing, "routes without a case in tests/helpers/attn_cases.py:\n" + "\n".join(missing)
    # the device-seed routes: one per (R4, C, flag) with dropout, and the GPU test takes its list from the same table
    dseed_have = {T.route_key(T.route(c, dseed=True)) for c in T.dseed_cases()}
    assert {k for k in grid_routes if k[6]} == dseed_have
    # UNREACHED: nothing in it is reported, and each entry is still a combination the dispatch could name
    reported = {k[:4] for k in grid_routes}
    assert not set(UNREACHED) & reported, "UNREACHED is stale: the routing reports " + str(sorted(set(UNREACHED) & reported))
    inst = source_instances()
    for fam, r4, cf, pieces in UNREACHED:
        assert (r4, cf) in inst and fam == 1 and r4 <= 8 and pieces in (2, 3), "UNREACHED is stale"
    want = {(fam, r4, cf, pieces) for (r4, cf) in inst for fam, pieces in ((0, 0), (1, 2), (1, 3)) if fam == 0 or r4 <= 8}
    assert reported | set(UNREACHED) == want, (sorted(want - reported - set(UNREACHED)), sorted(reported - want))


def source_instances():
    """(R4, CF) of every attn_launch<R4, CF, DSEED> that attn_dispatch_c names, for each R4 attn_dispatch instantiates it with"""
    src = open(SRC).read()
    body = src[src.index("static void attn_dispatch_c("):]
    body = body[:body.index("\n}\n")]
    rows = re.findall(r"(?:case (\d+)|default): attn_launch<R4, (\d+), DSEED>", body)
    assert len(rows) == 7 and body.count("attn_launch<") == 7, "attn_dispatch_c not understood"
    cfs = []
    for c, cf in rows:
        assert c == "" or int(c) == 16 * int(cf), (c, cf)
        cfs.append(int(cf))
    body = src[src.index("static void attn_dispatch("):]
    body = body[:body.index("\n}\n")]
    r4s = [int(r) for r in re.findall(r"attn_dispatch_c<(\d+), DSEED>", body)]
    assert len(r4s) == 4 and body.count("attn_dispatch_c<") == 4, "attn_dispatch not understood"
    assert sorted(int(r) for r in re.findall(r"attn_stats_kernel<(\d+)>", body)) == sorted(r4s)
    # no launch outside the dispatch functions
    assert src.count("attn_launch<") == 7 and src.count("attn_dispatch_c<") == 4
    return {(r4, cf) for r4 in r4s for cf in cfs}


def test_every_kernel_instance_is_reached_in_each_family():
    inst = source_instances()
    assert len(inst) == 28
    lib = __import__("buctd_amd._C", fromlist=["lib"]).lib()
    assert {(r4, c // 16) for r4 in range(1, 33) for c in range(1, 300) if lib.buctd_attn_smallqk_supported(128, r4, c)} == inst
    reached = {}
    for c in T.CASES:
        pl = T.route(c)
        reached.setdefault((pl["R4"], pl["CF"], pl["split"], pl["pieces"]), set()).add(pl["drop"])
    for r4, cf in sorted(inst):
        fams = [(0, 0)] + ([(1, 2)] + ([(1, 3)] if cf <= 8 else []) if r4 <= 8 else [])
        for fam, pieces in fams:
            got = reached.get((r4, cf, fam, pieces), set())
            assert got == {0, 1}, f"attn_launch<{r4}, {cf}> family {fam} pieces {pieces}: reached with DROP in {sorted(got)}"
    # every input family on every (kernel family, pieces, CF)
    fams = {}
    for c in T.CASES:
        pl = T.route(c)
        fams.setdefault((pl["split"], pl["pieces"], pl["CF"]), set()).add(c.inputs)
    assert len(fams) == 7 + 7 + 6
    short = {k: sorted(set(T.FAMILIES) - v) for k, v in fams.items() if v != set(T.FAMILIES)}
    assert not short, f"(family, pieces, CF) without an input family: {short}"


def test_query_and_launch_refuse_the_same_arguments():
    from buctd_amd import _C
    lib = _C.lib()
    out = (C.c_int * len(T.PLAN_FIELDS))()
    nan = float("nan")
    good = (128, 8, 64, 2, 0.3)
    assert T.plan(*good, False) is not None
    bad = [(100, 8, 64, 2, 0.3), (0, 8, 64, 2, 0.3), (-64, 8, 64, 2, 0.3), (128, 12, 64, 2, 0.3), (128, 5, 64, 2, 0.3),
           (128, 24, 64, 0, 0.0), (128, 8, 40, 2, 0.3), (128, 8, 256, 0, 0.0), (128, 8, 0, 1, 0.3), (128, 8, 64, 2, 1.0),
           (128, 8, 64, 0, 1.5), (128, 8, 64, 1, -0.1), (128, 8, 64, 2, nan), (128, 8, 64, 0, float("inf"))]
    # the pointers are never dereferenced: every call below returns before a launch
    for t, r4, c, flag, p in bad:
        for dseed in (0, 1):
            for i in range(len(out)):
                out[i] = 7
            assert lib.buctd_attn_smallqk_plan(t, r4, c, flag, p, dseed, out) == EINVAL, (t, r4, c, flag, p)
            assert list(out) == [0] * len(T.PLAN_FIELDS)
            assert b"buctd_attn_smallqk_plan" in lib.buctd_last_error()
            fwd = lib.buctd_attn_smallqk_fwd_dseed if dseed else lib.buctd_attn_smallqk_fwd
            bwd = lib.buctd_attn_smallqk_bwd_dseed if dseed else lib.buctd_attn_smallqk_bwd
            seed = BASE if dseed else T.SEED
            assert fwd(2, t, r4, c, BASE, BASE, BASE, 0.125, p, seed, flag, BASE, BASE, BASE, None) == EINVAL, (t, r4, c, flag, p)
            msg_f = lib.buctd_last_error()
            assert bwd(2, t, r4, c, *([BASE] * 7), 0.125, p, seed, flag, BASE, BASE, BASE, BASE, None) == EINVAL, (t, r4, c, flag, p)
            msg_b = lib.buctd_last_error()
            # the same message form in both directions, before anything is launched
            name_f = b"buctd_attn_smallqk_fwd" + (b"_dseed" if dseed else b"")
            name_b = b"buctd_attn_smallqk_bwd" + (b"_dseed" if dseed else b"")
            assert msg_f.startswith(name_f + b": ") and msg_b.startswith(name_b + b": ")
            assert msg_f[len(name_f):] == msg_b[len(name_b):], (msg_f, msg_b)
            assert (b"bad p_drop / size" in msg_f) == (T.plan(t, r4, c, flag, 0.0, False) is not None)
    # B * T past 2^31: the launches refuse what the query (which knows no B) cannot see
    assert lib.buctd_attn_smallqk_fwd(1 << 25, 64, 8, 64, BASE, BASE, BASE, 0.125, 0.0, 0, 0, BASE, BASE, BASE, None) == EINVAL
    assert b"bad p_drop / size" in lib.buctd_last_error()
    assert lib.buctd_attn_smallqk_bwd(1 << 25, 64, 8, 64, *([BASE] * 7), 0.125, 0.0, 0, 0, BASE, BASE, BASE, BASE, None) == EINVAL
    assert b"bad p_drop / size" in lib.buctd_last_error()
    # null arguments
    assert lib.buctd_attn_smallqk_plan(*good, 0, None) == EINVAL
    assert lib.buctd_attn_smallqk_fwd_dseed(2, 128, 8, 64, BASE, BASE, BASE, 0.125, 0.3, None, 2, BASE, BASE, BASE, None) == EINVAL
    assert lib.buctd_attn_smallqk_bwd(2, 128, 8, 64, *([BASE] * 7), 0.125, 0.3, 1, 2, BASE, BASE, BASE, None, None) == EINVAL
    assert lib.buctd_attn_smallqk_bwd(0, 128, 8, 64, *([BASE] * 7), 0.125, 0.3, 1, 2, BASE, BASE, BASE, BASE, None) == EINVAL


# ---- the input families, on the fp64 reference alone ------------------------------------------------------------------------
def test_rising_moves_the_maximum_in_every_tile_and_falling_fixes_it():
    seen = {"rising": 0, "falling": 0}
    for c in T.CASES:
        if c.inputs not in seen:
            continue
        seen[c.inputs] += 1
        s = T.reference(c)["s"]                                           # [B][T][T] scaled logits
        tile_max = s.view(T.B, c.T, c.T // 64, 64).amax(-1)               # per row, per 64-key tile
        if c.inputs == "rising":
            if c.T > 64:
                assert bool((tile_max[..., 1:] > tile_max[..., :-1]).all()), f"{T.case_id(c)}: a tile leaves the maximum where it was"
            # the statistics kernel walks key by key: its s > mx branch runs in every tile too (at T = 64 this is the condition)
            run = s.cummax(-1).values
            moved = (run[..., 1:] > run[..., :-1]).view(T.B, c.T, -1)
            per_tile = torch.nn.functional.pad(moved, (1, 0), value=True).view(T.B, c.T, c.T // 64, 64).any(-1)
            assert bool(per_tile.all()), T.case_id(c)
            assert int(moved.sum(-1).min()) >= c.T // 64 + 2
        else:
            assert bool((tile_max[..., :1] >= tile_max).all()) and bool((s.argmax(-1) < 64).all()), T.case_id(c)
        assert float(s.abs().max()) <= 40.0, T.case_id(c)
    assert min(seen.values()) >= 60


def test_peaked_rows_are_near_one_hot_with_centred_logits():
    n = 0
    for c in T.CASES:
        if c.inputs != "peaked":
            continue
        n += 1
        ref = T.reference(c)
        top = ref["P"].amax(-1)
        assert float(top.min()) >= 0.99, f"{T.case_id(c)}: largest probability of a row {float(top.min()):.4f}"
        assert float(ref["s"].abs().max()) <= 40.0, T.case_id(c)
        # the peaks lie in different tiles (where T allows) and every group of rows is present in both images
        peaks = ref["P"].argmax(-1)
        assert all(set(peaks[b].tolist()) == set(T.peak_keys(c.T, c.R4)) for b in range(T.B)), T.case_id(c)
        assert len(set(T.peak_keys(c.T, c.R4))) == c.R4 and len({j // 64 for j in T.peak_keys(c.T, c.R4)}) >= min(c.T // 64, c.R4, 4)
    assert n >= 60


def test_dropout_masks_are_live_and_no_row_is_empty():
    n = 0
    for c in T.CASES:
        mask = T.keep(c)
        if mask is None:
            continue
        n += 1
        assert bool((mask.sum(-1) > 0).all()), f"{T.case_id(c)}: a row with every key dropped"
        frac = mask.mean((1, 2))
        assert bool(((frac - (1 - c.p)).abs() <= 0.03).all()), f"{T.case_id(c)}: kept fractions {frac.tolist()}"
        assert not torch.equal(mask[0], mask[1])
    assert n >= 84 + 28


def test_no_reference_tensor_has_zero_norm_and_fp32_bars_are_finite():
    for c in T.CASES:
        ref = T.reference(c)
        for name in T.NAMES:
            assert float(ref[name].norm()) > 0 and float(ref[name].abs().max()) > 0 and bool(torch.isfinite(ref[name]).all()), \
                f"{T.case_id(c)}: {name}"
        for pieces in (0, 2, 3):
            for name, (b2, bm) in T.bars(c, pieces).items():
                assert T.PROJECT_BAR[pieces] <= b2 < 1e-3 and T.PROJECT_BAR[pieces] <= bm < 1e-3, (T.case_id(c), name, b2, bm)
            if c.inputs == "gaussian":
                assert set(T.bars(c, pieces).values()) == {(T.PROJECT_BAR[pieces],) * 2}
