"""Closure of the group table (tests/helpers/c3_group_cases.py) over what a 3x3 bf16x6 group launch can run (host only: the
queries buctd_conv3x3_bf16x6_group_plan / buctd_conv3x3_wgrad_bf16x6_group_plan report the descriptor the launch hands to its
kernel, without a launch).

A group launch has code no single launch runs: the workgroup -> (member, tile) walk over the eight XCDs, the cost order of the
members, the search for a common kernel family, a variant per member, the LDS size of the largest member; in the weight
gradient the first[] lookup, a split count per member and a shared reduction.  This module proves that the table reaches every
kernel variant as a member of a multi-member group, restates the walk in plain Python on the query's figures, and says by name
which shape sets of tests/test_gpu_branches.py really form one train-mode kernel."""
import ctypes as C

import pytest

from tests.helpers import c3_cases as T
from tests.helpers import c3_group_cases as G
from tests.test_conv3x3_plan_cover import LEAN_SETS, conv_key, source_instances, wgrad_key

ALL_GROUPS = [(opt, name) for opt in T.OPTION_SETS for name in G.conv_groups(opt)]


def _plan(opt, name):
    return G.group_plan(G.conv_groups(opt)[name], T.OPTION_SETS[opt])


def test_table_has_the_groups_the_closure_relies_on():
    """a group removed from the table fails here, by name"""
    assert list(G.TRAIN_GROUPS) == ["f1", "f1-col", "f1-v0v2", "f0", "f0-col", "f1-twins"]
    assert list(G.EVAL_GROUPS) == ["eval-v6", "eval-v7"]
    assert list(G.WGRAD_GROUPS) == ["cf3-n2", "cf3-n3", "cf3-n4", "cf2-n2", "cf2-n3"]
    assert {len(s) for s in G.TRAIN_GROUPS.values()} == {2, 3, 4}
    for name, shapes in {**G.TRAIN_GROUPS, **G.EVAL_GROUPS}.items():
        for s in shapes:
            assert conv_key(s, -1) is not None, f"{name}: {s} is unsupported"


@pytest.mark.parametrize("opt,name", ALL_GROUPS, ids=lambda v: v)
def test_every_group_forms_one_kernel_of_its_option_set(opt, name):
    p = _plan(opt, name)
    assert p["one_kernel"], f"{name} under {opt}: the members go out one launch each - the group tests would test nothing"
    assert p["option_set"] == T.OPTION_SETS[opt]
    assert sorted(m["index"] for m in p["members"]) == list(range(len(p["members"])))


def test_eval_only_and_no_family_groups_under_the_train_option_sets():
    for m in LEAN_SETS:
        for name, shapes in G.EVAL_GROUPS.items():
            assert not G.group_plan(shapes, m)["one_kernel"], f"{name} forms a train-mode kernel under option set {m}: move it"
        p = G.group_plan(G.NO_FAMILY_GROUP, m)
        assert not p["one_kernel"] and p["members"] == [], f"option set {m}: must report one launch per member"
        assert G.group_workgroups(G.NO_FAMILY_GROUP, m) == 0


def test_table_reaches_every_variant_as_a_member_of_a_group():
    """every (family, variant) of the train-mode tables under each of the five option sets, every variant of the general group
    kernel in both families - a variant added to a family table in the source fails here, by name"""
    inst, tabs = source_instances()
    got = G.reached_instances()
    n_train = {f: 1 + max(v for (k, m, ff, v) in (i for i in inst if i[0] == "lean") if ff == f) for f in (0, 1)}
    want = {("lean", m, f, v) for m in LEAN_SETS for f in (0, 1) for v in range(n_train[f])}
    want |= {("group", f, v) for f in (0, 1) for v in range(len(tabs[f]))}
    missing = sorted(want - got)
    assert not missing, f"kernel variants that no multi-member group of the table runs: {missing}"
    assert got <= want, f"the query reports variants the source tables do not have: {sorted(got - want)}"


@pytest.mark.parametrize("opt,name", ALL_GROUPS, ids=lambda v: v)
def test_query_variants_are_the_indices_of_the_source_tables(opt, name):
    _, tabs = source_instances()
    shapes = G.conv_groups(opt)[name]
    p = _plan(opt, name)
    for mem in p["members"]:
        s = shapes[mem["index"]]
        kernel, MF, NF, WM, WN, single, col, fam, var = conv_key(s, -1)
        assert tabs[p["family"]][mem["variant"]] == (MF, NF, WM, WN), f"{name} {opt}: member {mem['index']} {s}"
        assert mem["col_major"] == col
        # gx, gy from the member's own plan
        out = (C.c_int * 11)()
        from buctd_amd import _C
        assert _C.lib().buctd_conv3x3_bf16x6_plan(*s, -1, out) == 0
        N, H, W, Ci, Co = s
        P = N * (H + 1) * (W + 1) + W + 1
        assert mem["gx"] == -(-P // out[9]) and mem["gy"] == Co // out[10] and mem["tiles"] == mem["gx"] * mem["gy"]


def walk(tiles, lin):
    """the (member, tile) of workgroup lin: the loop of conv3x3_x6_group_kernel / conv3x3_x6_lean_kernel, restated"""
    xcd, idx = lin & 7, lin >> 3
    for k, total in enumerate(tiles):
        per, rem = total >> 3, total & 7
        mine = per + (1 if xcd < rem else 0)
        if idx < mine:
            return k, (xcd * (per + 1) + idx if xcd < rem else rem * (per + 1) + (xcd - rem) * per + idx)
        idx -= mine
    return None


@pytest.mark.parametrize("opt,name", ALL_GROUPS, ids=lambda v: v)
def test_grid_and_walk_visit_every_tile_exactly_once(opt, name):
    p = _plan(opt, name)
    tiles = [m["tiles"] for m in p["members"]]
    assert p["grid"] == 8 * sum(-(-t // 8) for t in tiles), f"{name} {opt}: grid {p['grid']} for tiles {tiles}"
    seen = {}
    idle = 0
    for lin in range(p["grid"]):
        r = walk(tiles, lin)
        if r is None:
            idle += 1
            continue
        k, L = r
        assert 0 <= L < tiles[k], f"{name} {opt}: workgroup {lin} gets tile {L} of member {k} ({tiles[k]} tiles)"
        assert (k, L) not in seen, f"{name} {opt}: workgroups {seen[(k, L)]} and {lin} both compute tile {L} of member {k}"
        seen[(k, L)] = lin
        m = p["members"][k]
        bx, by = (L % m["gx"], L // m["gx"]) if m["col_major"] else (L // m["gy"], L % m["gy"])
        assert 0 <= bx < m["gx"] and 0 <= by < m["gy"]
    assert len(seen) == sum(tiles) and idle == p["grid"] - sum(tiles)


@pytest.mark.parametrize("opt,name", ALL_GROUPS, ids=lambda v: v)
def test_launch_order_is_by_tile_cost_and_lds_is_the_largest_members(opt, name):
    shapes = G.conv_groups(opt)[name]
    p = _plan(opt, name)
    from buctd_amd import _C
    costs, lds = [], []
    for mem in p["members"]:
        s = shapes[mem["index"]]
        out = (C.c_int * 11)()
        assert _C.lib().buctd_conv3x3_bf16x6_plan(*s, -1, out) == 0
        costs.append(out[9] * out[10] * s[3])             # BM * BN * Ci
        if T.OPTION_SETS[opt] >= 0:
            one = G.group_plan([s], T.OPTION_SETS[opt])      # a train-mode launch of the member alone: its own LDS size
            assert one["one_kernel"]
            lds.append(one["lds"])
    assert costs == sorted(costs, reverse=True), f"{name} {opt}: launch order {costs} is not non-increasing in BM * BN * Ci"
    # equal costs keep the call order
    for a, b, ca, cb in zip(p["members"], p["members"][1:], costs, costs[1:]):
        assert ca != cb or a["index"] < b["index"]
    if lds:
        assert p["lds"] == max(lds), f"{name} {opt}: LDS {p['lds']} but the members need {lds}"


def test_table_properties():
    tiles_mod8, not_cost_order, equal_cost, big_lds_not_first = set(), 0, 0, 0
    from buctd_amd import _C
    for name, shapes in G.TRAIN_GROUPS.items():
        p = G.group_plan(shapes, T.C3M_STATS)
        tiles_mod8 |= {m["tiles"] % 8 for m in p["members"]}
        order = [m["index"] for m in p["members"]]
        costs = []
        for s in shapes:
            out = (C.c_int * 11)()
            assert _C.lib().buctd_conv3x3_bf16x6_plan(*s, -1, out) == 0
            costs.append(out[9] * out[10] * s[3])
        equal_cost += len(set(costs)) < len(costs)
        if len(set(costs)) == len(costs):
            assert order != list(range(len(shapes))), f"{name}: the members are given in their launch order"
            not_cost_order += 1
        lds = [G.group_plan([shapes[i]], T.C3M_STATS)["lds"] for i in order]
        big_lds_not_first += lds.index(max(lds)) != 0
    assert {0, 1, 7} <= tiles_mod8, f"tiles % 8 of the members: {sorted(tiles_mod8)}"
    assert not_cost_order >= 4 and equal_cost >= 1 and big_lds_not_first >= 1
    assert any(any(m["col_major"] for m in G.group_plan(s, T.C3M_STATS)["members"]) and
               not all(m["col_major"] for m in G.group_plan(s, T.C3M_STATS)["members"]) for s in G.TRAIN_GROUPS.values())


def test_workgroups_query_agrees_with_the_plan_query():
    for opt, name in ALL_GROUPS:
        shapes = G.conv_groups(opt)[name]
        assert G.group_workgroups(shapes, T.OPTION_SETS[opt]) == _plan(opt, name)["grid"] > 0, f"{name} {opt}"
    for m in list(LEAN_SETS) + [-1]:
        p = G.group_plan(G.NO_FAMILY_GROUP, m)
        assert G.group_workgroups(G.NO_FAMILY_GROUP, m) == (p["grid"] if p["one_kernel"] else 0)


def test_eval_branches_ok_memoises_what_the_query_says(monkeypatch):
    """ops.eval_branches_ok asks buctd_conv3x3_bf16x6_group_workgroups with option-free entries: the plan of the eval call"""
    import torch
    from buctd_amd import ops

    class FakeX:                      # what eval_branches_ok reads of an activation, without a device
        is_cuda, dtype = True, torch.float32

        def __init__(self, shape):
            self.shape = torch.Size(shape)

        def dim(self):
            return 4

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return C.addressof(G._SOME)

    class FakeW:
        def __init__(self, Cn):
            self.shape = torch.Size((Cn, Cn, 3, 3))

    monkeypatch.setattr(ops, "_bf16x3_ok", lambda d: True)
    monkeypatch.setattr(ops, "_wshape", lambda w: tuple(w.shape))
    monkeypatch.setitem(ops._conv_math, "mode", "bf16x6")
    sets = [[(s[0], s[1], s[2], s[3]) for s in shapes] for shapes in
            (G.EVAL_GROUPS["eval-v6"], G.NO_FAMILY_GROUP, [(1, 8, 6, 48), (1, 2, 2, 384)])]
    sets += [sh for sh, _ in G.BRANCH_TEST_SHAPES.values()]
    for nhwc in sets:
        xs = [FakeX(s) for s in nhwc]
        chains = [[(FakeW(s[3]), None, FakeW(s[3]), None)] for s in nhwc]
        full = [s + (s[3],) for s in nhwc]
        assert ops.eval_branches_ok(xs, chains) == (G.group_workgroups(full, -1) > 0) == G.group_plan(full, -1)["one_kernel"], nhwc


@pytest.mark.parametrize("name", list(G.BRANCH_TEST_SHAPES))
def test_which_branch_tests_form_one_train_mode_kernel(name):
    """tests/test_gpu_branches.py asserts "group == chains, bit for bit".  Where the branches share no train-mode kernel the
    group entry point launches each member on its own, and that assertion compares the same launches on both sides.  If a plan
    change flips one of these, this test says which guarantee moved."""
    nhwc, one = G.BRANCH_TEST_SHAPES[name]
    shapes = [s + (s[3],) for s in nhwc]
    for m in LEAN_SETS:
        assert G.group_plan(shapes, m)["one_kernel"] == one, \
            f"{name}: option set {m} {'no longer forms' if one else 'now forms'} one train-mode kernel"


def test_branch_test_shapes_are_those_of_the_gpu_module():
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_branches.py")).read()
    tree = ast.parse(src)
    found = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == "test_branches_node_equals_chains":
            call = node.decorator_list[0]
            sets = ast.literal_eval(call.args[1])
            ids = ast.literal_eval([k.value for k in call.keywords if k.arg == "ids"][0])
            found.update(zip(ids, sets))
    assert found, "test_branches_node_equals_chains not understood"
    for k, v in found.items():
        assert k in G.BRANCH_TEST_SHAPES and G.BRANCH_TEST_SHAPES[k][0] == v, f"shape set {k} of test_gpu_branches.py is not in the table"
    assert "shapes = [(2, 8, 6, 32), (2, 4, 3, 64)]" in src and \
        "torch.randn(2, 16, 12, 48, device=dev), torch.randn(2, 8, 6, 96, device=dev), torch.randn(2, 4, 3, 192, device=dev)" in src


# ---- weight gradient ------------------------------------------------------------------------------------------------------
def test_weight_gradient_groups_reach_every_key_and_both_reductions():
    keys, cfs, sizes = set(), set(), set()
    target = 256
    small = ragged = mixed_acc = some_bn = rem_mix = False
    for name, members in G.WGRAD_GROUPS.items():
        r = G.wgrad_group_plan(members)
        assert r is not None, f"{name} is refused"
        plans, grid, lds = r
        cf = {p["CF"] for p in plans}
        assert len(cf) == 1
        cfs |= cf
        sizes.add((cf.pop(), len(members)))
        first = 0
        fp = 0
        for p, (s, acc, x_bn) in zip(plans, members):
            keys.add((p["CF"], p["nsplit"] == 1, p["rem"] == 0))
            assert p["first"] == first and p["first_pair"] == fp, f"{name}: {s}"
            first += p["pairs"] * p["nsplit"]
            fp += p["pairs"]
            N, H, W, Ci, Co = s
            ch = 16 * p["CF"]
            assert p["pairs"] == (Co // ch) * -(-Ci // ch)
            stages = p["nsplit"] * p["q"] + p["rem"]
            want = -(-target // p["pairs"])
            assert p["nsplit"] == min(want, stages) and 0 <= p["rem"] < p["nsplit"], f"{name}: {s} {p}"
            small |= stages < want
            ragged |= Ci % ch != 0
            if x_bn:
                assert Ci % ch == 0, f"{name}: {s} has x_bn but a ragged input chunk"
            # the single launch splits for the whole chip: the group must not simply reuse its plan
            assert wgrad_key(s) is not None
        assert grid == first
        mixed_acc |= len({a for _, a, _ in members}) == 2
        some_bn |= len({b for _, _, b in members}) == 2
        rem_mix |= len({p["rem"] == 0 for p in plans}) == 2
    assert cfs == {2, 3}, "both reduction kernels (wg3_reduce_group_kernel<2> and <3>)"
    assert {(3, 2), (3, 3), (3, 4), (2, 2), (2, 3)} <= sizes
    want_keys = {(cf, one, rem0) for cf in (2, 3) for one, rem0 in ((True, True), (False, True), (False, False))}
    assert want_keys <= keys, f"weight-gradient keys (CF, nsplit == 1, rem == 0) no group reaches: {sorted(want_keys - keys)}"
    assert small and ragged and mixed_acc and some_bn and rem_mix
    assert any(s == (17, 2, 74, 64, 48) for ms in G.WGRAD_GROUPS.values() for s, _, _ in ms)


def test_weight_gradient_group_queries_agree_and_refuse_mixed_chunk_widths():
    from buctd_amd import _C
    for name, members in G.WGRAD_GROUPS.items():
        plans, grid, lds = G.wgrad_group_plan(members)
        assert _C.lib().buctd_conv3x3_wgrad_bf16x6_group_workgroups(len(members), G.wgrad_items(members)) == grid
        for p, (s, _, _) in zip(plans, members):
            assert _C.lib().buctd_conv3x3_wgrad_bf16x6_group_workspace(len(members), *s) == p["ws_bytes"]
    assert G.wgrad_group_plan(G.WGRAD_MIXED_CF) is None
    # one member: the single launch's plan
    s = (3, 7, 5, 48, 96)
    plans, grid, _ = G.wgrad_group_plan([(s, 0, False)])
    out = (C.c_int * 4)()
    assert _C.lib().buctd_conv3x3_wgrad_bf16x6_plan(*s, out) == 0
    assert [plans[0][k] for k in ("CF", "nsplit", "q", "rem")] == list(out) and grid == plans[0]["pairs"] * plans[0]["nsplit"]
