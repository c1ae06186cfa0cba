"""The group launches of the 3x3 bf16x6 convolution tests, as data: which members share a launch
(buctd_conv3x3_bf16x6_group / _group_eval, buctd_conv3x3_wgrad_bf16x6_group), and the no-launch queries that say what such a
launch would run (buctd_conv3x3_bf16x6_group_plan, buctd_conv3x3_wgrad_bf16x6_group_plan).

A member is a shape (N, H, W, Ci, Co) of tests/helpers/c3_cases.py - ONE kernel call, Ci -> Co, whichever option set runs it.
tests/test_conv3x3_group_cover.py (host only) proves what the table reaches; tests/test_gpu_conv3x3_groups.py runs it."""
import ctypes as C

from tests.helpers import c3_cases as T

# ---- convolution groups: name -> members in CALL order (never the launch order: the launch sorts by tile cost) ------------
# comment: family; the variants in call order; tiles % 8 of the members
TRAIN_GROUPS = {
    "f1":        [(33, 31, 25, 16, 64), (36, 31, 25, 16, 64), (33, 23, 19, 16, 128), (2, 7, 5, 16, 32)],   # 1; 1, 4, 5, 3; 6, 3, 0, 2
    "f1-col":    [(1, 7, 5, 384, 192), (33, 3, 73, 384, 256), (36, 31, 25, 16, 64)],        # 1; 3 col, 5 col, 4; 6, 4, 3; Ci > Co
    # the 128 x 32 and 256 x 32 tiles live in both families: a member that only family 1 has takes them there
    "f1-v0v2":   [(32, 12, 9, 16, 160), (32, 17, 13, 16, 160), (11, 7, 5, 16, 32)],         # 1; 2, 0, 3; 5, 0, 1
    "f0":        [(21, 95, 71, 16, 48), (36, 31, 25, 96, 96), (33, 1, 37, 16, 256), (36, 47, 35, 16, 48)],  # 0; 0, 1, 2, 3; H = 1
    "f0-col":    [(33, 2, 74, 16, 192), (33, 2, 74, 192, 384), (33, 29, 1, 192, 384), (17, 2, 74, 192, 384)],   # 0; 4, 1 col, 2 col, 4 col
    "f1-twins":  [(8, 7, 5, 16, 32), (8, 7, 5, 16, 32)],                                    # 1; 3, 3: equal cost; 7, 7
}
# groups that share a kernel only in the eval entry point (the 48-column tiles of the general group kernel's family 1)
EVAL_GROUPS = {
    "eval-v6":   [(1, 8, 6, 48, 48), (1, 4, 3, 96, 96)],                                    # 1; 6, 3
    "eval-v7":   [(16, 48, 36, 16, 48), (16, 24, 18, 96, 96)],                              # 1; 7, 2
}
# no kernel family holds the tiles of both members under a train-mode option set: one launch per member
NO_FAMILY_GROUP = [(3, 24, 18, 48, 48), (3, 12, 9, 96, 96)]


def conv_groups(option_name):
    """{name: members} of the groups that run under this option set ("general" = the eval entry point)"""
    g = dict(TRAIN_GROUPS)
    if option_name == "general":
        g.update(EVAL_GROUPS)
    return g


# ---- the shape sets of tests/test_gpu_branches.py (N, H, W, C per branch) and whether their branch convolutions form ONE
# train-mode kernel; tests/test_conv3x3_group_cover.py asserts it by name ------------------------------------------------------
BRANCH_TEST_SHAPES = {
    "w48x2":    ([(3, 24, 18, 48), (3, 12, 9, 96)], False),
    "w48x4":    ([(2, 24, 20, 48), (2, 12, 10, 96), (2, 6, 5, 192), (2, 3, 3, 384)], False),
    "w32x3":    ([(2, 16, 12, 32), (2, 8, 6, 64), (2, 4, 3, 128)], True),
    "w48_full": ([(32, 96, 72, 48), (32, 48, 36, 96), (32, 24, 18, 192), (32, 12, 9, 384)], True),
    "unused_branch": ([(2, 8, 6, 32), (2, 4, 3, 64)], True),
    "module":   ([(2, 16, 12, 48), (2, 8, 6, 96), (2, 4, 3, 192)], False),
}

# ---- weight-gradient groups: name -> members (shape, accumulate, x_bn) in call order ---------------------------------------
# x_bn members need whole input chunks (Ci % (16 CF) == 0)
WGRAD_GROUPS = {
    "cf3-n2":      [((3, 7, 5, 48, 96), 0, False), ((1, 6, 5, 96, 48), 1, True)],            # a member with stages < target
    "cf3-n3":      [((2, 12, 9, 48, 48), 0, False), ((8, 31, 25, 96, 96), 0, False), ((2, 3, 3, 192, 192), 0, False)],   # rem != 0 in the middle
    "cf3-n4":      [((17, 2, 74, 64, 48), 1, False), ((5, 1, 37, 48, 48), 0, True), ((3, 7, 5, 48, 96), 0, False),
                    ((17, 2, 74, 96, 48), 1, True)],                                         # ragged last input chunk (Ci = 64)
    "cf2-n2":      [((20, 3, 73, 32, 192), 0, True), ((1, 6, 5, 32, 64), 1, False)],
    "cf2-n3":      [((2, 7, 5, 64, 32), 1, True), ((20, 3, 73, 32, 192), 0, False), ((2, 7, 5, 64, 32), 0, False)],
}
WGRAD_MIXED_CF = [((3, 7, 5, 48, 96), 0, False), ((2, 7, 5, 64, 32), 0, False)]       # refused: 48- and 32-channel chunks


# ---- the queries ----------------------------------------------------------------------------------------------------------
_SOME = (C.c_float * 4)()         # stands for "this pointer is set": the queries read nothing through it


def _on():
    return C.addressof(_SOME)


def conv_items(shapes, option_set):
    """(_C.C3Conv * n) as buctd_conv3x3_bf16x6_group would get them for this option set (C3M_* mask, -1: none = the entries
    of buctd_conv3x3_bf16x6_group_eval), with placeholder pointers; the second value keeps what the items point to alive"""
    from buctd_amd import _C
    items = (_C.C3Conv * len(shapes))()
    keep = []
    for it, s in zip(items, shapes):
        it.N, it.H, it.W, it.Ci, it.Co = s
        it.x = it.wprep = it.y = _on()
        if option_set < 0:
            continue
        if option_set & T.C3M_STATS:
            it.stats_acc = _on()
        if option_set & T.C3M_IN_BN:
            b = _C.BnAccIn()
            b.acc, b.rows, b.eps, b.momentum, b.mean_out, b.invstd_out = _on(), 1, 1e-5, 0.1, _on(), _on()
            keep.append(b)
            it.in_bn = C.pointer(b)
            it.in_gamma = it.in_beta = _on()
            it.in_relu = 1
        if option_set & T.C3M_RES:
            it.residual = _on()
        if option_set & (T.C3M_BS_REBUILD | T.C3M_BS_Y):
            it.bn_acc = it.bn_z = it.bn_mean = it.bn_invstd = it.bn_gamma = _on()
            if option_set & T.C3M_BS_Y:
                it.bn_y = _on()
            else:
                it.bn_beta = _on()
    return items, keep


PLAN_INTS = 30


def group_plan(shapes, option_set):
    """buctd_conv3x3_bf16x6_group_plan as a dict: one_kernel, option_set, family, grid, lds, members = [dict(index, variant,
    gx, gy, tiles, col_major)] in LAUNCH order ([] when the members go out one launch each)"""
    from buctd_amd import _C
    items, keep = conv_items(shapes, option_set)
    out = (C.c_int * PLAN_INTS)()
    rc = _C.lib().buctd_conv3x3_bf16x6_group_plan(len(shapes), items, out)
    assert rc == 0, f"buctd_conv3x3_bf16x6_group_plan{tuple(shapes)}: error {rc}"
    v = list(out)
    assert v[5] == len(shapes)
    members = []
    if v[0]:
        for i in range(len(shapes)):
            members.append(dict(zip(("index", "variant", "gx", "gy", "tiles", "col_major"), v[6 + 6 * i:12 + 6 * i])))
    return dict(one_kernel=bool(v[0]), option_set=v[1], family=v[2], grid=v[3], lds=v[4], members=members)


def group_workgroups(shapes, option_set):
    from buctd_amd import _C
    items, keep = conv_items(shapes, option_set)
    return _C.lib().buctd_conv3x3_bf16x6_group_workgroups(len(shapes), items)


def wgrad_items(members):
    from buctd_amd import _C
    items = (_C.Wg3Conv * len(members))()
    for it, (s, accumulate, x_bn) in zip(items, members):
        it.N, it.H, it.W, it.Ci, it.Co = s
        it.accumulate = accumulate
        if x_bn:
            it.x_mean = it.x_invstd = it.x_gamma = it.x_beta = _on()
            it.x_relu = 1
    return items


WG_PLAN_INTS = 34


def wgrad_group_plan(members):
    """buctd_conv3x3_wgrad_bf16x6_group_plan: ([dict(CF, nsplit, q, rem, first, pairs, first_pair, ws_bytes)] per member in
    call order, grid, lds), or None where the call is refused"""
    from buctd_amd import _C
    out = (C.c_int * WG_PLAN_INTS)()
    if _C.lib().buctd_conv3x3_wgrad_bf16x6_group_plan(len(members), wgrad_items(members), out) != 0:
        return None
    v = list(out)
    names = ("CF", "nsplit", "q", "rem", "first", "pairs", "first_pair", "ws_bytes")
    return [dict(zip(names, v[8 * k:8 * k + 8])) for k in range(len(members))], v[32], v[33]


def group_id(name, option_name=None):
    return name if option_name is None else f"{name}-{option_name}"


def reached_instances():
    """the kernel instances (as tests/test_conv3x3_plan_cover.py names them) that a MULTI-member group of the table runs:
    ("lean", option set, family, variant) for the train-mode kernels, ("group", family, variant) for the general group kernel"""
    got = set()
    for opt_name, m in T.OPTION_SETS.items():
        for name, shapes in conv_groups(opt_name).items():
            p = group_plan(shapes, m)
            if p["one_kernel"] and len(shapes) > 1:
                for mem in p["members"]:
                    got.add(("lean", m, p["family"], mem["variant"]) if m >= 0 else ("group", p["family"], mem["variant"]))
    return got
