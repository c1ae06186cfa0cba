"""Closure of the 3x3 bf16x6 case table (tests/helpers/c3_cases.py) over the tile plans (host only: the plan queries
buctd_conv3x3_bf16x6_plan / buctd_conv3x3_wgrad_bf16x6_plan run the launch's own plan functions without a launch).

Every kernel variant that c3_plan / c3_lean_mode / c3_group_variant / wg3_plan can pick on the search grid must be reached by
a shape of the table - so a retuned threshold or a new variant without a test shape fails here, by name - and every kernel
instance in the source is either reached or listed in UNREACHED with the reason."""
import ctypes as C
import itertools
import os
import re

import pytest

from tests.helpers import c3_cases as T
from tests.helpers import c3_group_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "buctd_amd", "csrc")
LEAN_SETS = [m for m in T.OPTION_SETS.values() if m >= 0]


def conv_key(shape, option_set):
    """(kernel, MF, NF, WM, WN, single, col_major, family, variant), or None for an unsupported shape"""
    from buctd_amd import _C
    out = (C.c_int * 11)()
    if _C.lib().buctd_conv3x3_bf16x6_plan(*shape, option_set, out) != 0:
        return None
    v = list(out)
    return (v[6], v[0], v[1], v[2], v[3], v[4], v[5], v[7], v[8])


def wgrad_key(shape):
    """(CF, nsplit == 1, rem == 0), or None"""
    from buctd_amd import _C
    out = (C.c_int * 4)()
    if _C.lib().buctd_conv3x3_wgrad_bf16x6_plan(*shape, out) != 0:
        return None
    return (out[0], out[1] == 1, out[3] == 0)


def grid():
    for N, (H, W), Ci, Co in itertools.product(T.GRID_N, T.GRID_HW, T.GRID_C, T.GRID_C):
        yield (N, H, W, Ci, Co)


@pytest.fixture(scope="module")
def grid_keys():
    """{option set: {key: first grid shape}} and {wgrad key: first grid shape}"""
    conv = {m: {} for m in T.OPTION_SETS.values()}
    wg = {}
    for s in grid():
        for m in conv:
            k = conv_key(s, m)
            if k is not None:
                conv[m].setdefault(k, s)
        k = wgrad_key(s)
        if k is not None:
            wg.setdefault(k, s)
    return conv, wg


def source_instances():
    """The kernel instances conv3x3.hip can launch for NP = 3: ("x6", MF, NF, WM, WN) from the C3_CASE list of c3_dispatch,
    ("lean", option set, family, variant) from the family tables up to their train-mode length, ("group", 1, variant) for the
    entries of family 1 that only the general group kernel has."""
    src = open(os.path.join(CSRC, "conv3x3.hip")).read()
    body = src[src.index("static int c3_dispatch("):]
    body = body[:body.index("#undef C3_MF")]
    mfs = [int(m) for m in re.findall(r"C3_CASE\((\d+), nf, wm, wn\)", re.search(r"#define C3_MF\(nf, wm, wn\)(.*)", body).group(1))]
    assert mfs, "C3_MF not understood"
    lines = [l for l in body.splitlines() if not l.lstrip().startswith("#define") and not l.rstrip().endswith("\\")
             and "pl.MF ==" not in l]
    text = "\n".join(lines)
    inst = set()
    for mf, nf, wm, wn in re.findall(r"C3_CASE\((\d+), (\d+), (\d+), (\d+)\)", text):
        inst.add(("x6", int(mf), int(nf), int(wm), int(wn)))
    for nf, wm, wn in re.findall(r"C3_MF\((\d+), (\d+), (\d+)\)", text):
        inst.update(("x6", mf, int(nf), int(wm), int(wn)) for mf in mfs)
    tabs = {}
    for f in (0, 1):
        row = re.search(r"static const V f%d\[\] = \{(.*)\};" % f, src).group(1)
        tabs[f] = [tuple(int(v) for v in t) for t in re.findall(r"\{(\d+), (\d+), (\d+), (\d+)\}", row)]
    n1_general, n1_train = (int(v) for v in re.search(r"f \? \(general \? (\d+) : (\d+)\)", src).groups())
    assert len(tabs[1]) == n1_general and len(tabs[0]) == int(re.search(r"f \? \(general \? \d+ : \d+\) : (\d+)", src).group(1))
    for m in LEAN_SETS:
        inst.update(("lean", m, 0, v) for v in range(len(tabs[0])))
        inst.update(("lean", m, 1, v) for v in range(n1_train))
    inst.update(("group", 1, v) for v in range(n1_train, n1_general))
    return inst, tabs


# instances that no launch reaches from any grid shape, and why.  The only place where cases are left out.  (What only a group
# launch reaches - the 128 x 32 and 64 x 32 tiles as family-1 members, the 48-column tiles of the eval-mode group kernel - is
# reached by the group table, tests/helpers/c3_group_cases.py.)
UNREACHED = {
    ("x6", 8, 3, 2, 2): "dead: c3_plan takes the single-buffer tiles (MF = 7 / 8) only with wn == 1",
    ("x6", 1, 3, 2, 2): "dead: 2x2 waves with NF = 3 need >= 200 tiles of 128 positions per 96 columns (else the 32-column "
                        "tiles take over), and then MF = 2 always finds its 224 workgroups",
}

def reached_instances(conv):
    got = set()
    for m, keys in conv.items():
        for (kernel, MF, NF, WM, WN, single, col, fam, var) in keys:
            got.add(("x6", MF, NF, WM, WN) if kernel == 0 else ("lean", m, fam, var))
    return got


def test_plan_query_refuses_what_the_launch_refuses():
    from buctd_amd import _C
    assert conv_key((2, 8, 6, 48, 48), 2) is not None
    assert conv_key((2, 8, 6, 40, 48), 2) is None and conv_key((2, 8, 75, 48, 48), -1) is None      # Ci % 16, W > 74
    assert conv_key((2, 8, 6, 48, 48), 6) is None and conv_key((2, 8, 6, 48, 48), 0) is None        # STATS | RES, empty mask
    assert wgrad_key((2, 8, 6, 48, 48)) is not None and wgrad_key((2, 8, 1, 48, 48)) is None and wgrad_key((2, 8, 6, 16, 16)) is None
    for s in [(2, 8, 6, 48, 48), (32, 96, 72, 48, 48), (3, 17, 13, 96, 64)]:
        assert (conv_key(s, -1) is not None) == (_C.lib().buctd_conv3x3_bf16x6_supported(*s) == 1)
        # the row groups of the partial-sum statistics come from the same plan
        ng, rpg, out = C.c_int(), C.c_int(), (C.c_int * 11)()
        assert _C.lib().buctd_conv3x3_bf16x6_stats_groups(*s, C.byref(ng), C.byref(rpg)) == 0
        assert _C.lib().buctd_conv3x3_bf16x6_plan(*s, -1, out) == 0
        N, H, W = s[:3]
        P = N * (H + 1) * (W + 1) + W + 1
        assert rpg.value == out[0] * 16 and ng.value == -(-P // out[9]) * out[2] and out[9] == out[0] * out[2] * 16
        assert out[10] == out[1] * out[3] * 16


def test_every_plan_on_the_grid_has_a_case(grid_keys):
    conv, wg = grid_keys
    missing = []
    for name, m in T.OPTION_SETS.items():
        have = {conv_key(s, m) for s in T.CASES}
        assert None not in have, f"a case of the table is unsupported: {[s for s in T.CASES if conv_key(s, m) is None]}"
        for k, s in sorted(conv[m].items()):
            if k not in have:
                missing.append(f"{name}: (kernel, MF, NF, WM, WN, single, col_major, family, variant) = {k}, e.g. at {s}")
    have = {wgrad_key(s) for s in T.WGRAD_CASES}
    assert None not in have, f"unsupported weight-gradient case: {[s for s in T.WGRAD_CASES if wgrad_key(s) is None]}"
    for k, s in sorted(wg.items()):
        if k not in have:
            missing.append(f"wgrad: (CF, nsplit == 1, rem == 0) = {k}, e.g. at {s}")
    assert not missing, "plans without a test shape in tests/helpers/c3_cases.py:\n" + "\n".join(missing)


def test_model_shapes_are_supported_in_both_directions():
    for s in T.MODEL_CASES:
        N, H, W, Ci, Co = s
        for m in T.OPTION_SETS.values():
            assert conv_key(s, m) is not None, f"{s} forward, option set {m}"
            assert conv_key((N, H, W, Co, Ci), m) is not None, f"{s} as a data gradient, option set {m}"
        assert wgrad_key(s) is not None, f"{s} weight gradient"
    # the branch convolutions of the models run the train-mode kernels, not the fall-back
    for s in T.MODEL_CASES[:8]:
        for m in LEAN_SETS:
            assert conv_key(s, m)[0] == 1, f"{s}: option set {m} falls back to the general kernel"


def test_every_kernel_instance_is_reached_or_listed(grid_keys):
    conv, _ = grid_keys
    inst, tabs = source_instances()
    got = reached_instances(conv)
    assert got <= inst, f"the plan query reports kernels the source does not have: {sorted(got - inst)}"
    # the variant indices of the query are those of the tables
    for m, keys in conv.items():
        for (kernel, MF, NF, WM, WN, single, col, fam, var) in keys:
            if kernel == 1:
                assert tabs[fam][var] == (MF, NF, WM, WN), (m, fam, var)
    groups = G.reached_instances()
    assert groups <= inst | {("group", f, v) for f in tabs for v in range(len(tabs[f]))}, \
        f"the group query reports kernels the source does not have: {sorted(groups - inst)}"
    unlisted = sorted(inst - got - groups - set(UNREACHED))
    assert not unlisted, f"kernel instances that neither a grid shape nor a group of the table reaches and UNREACHED does not explain: {unlisted}"
    assert len(UNREACHED) == 2 and all(k[0] == "x6" for k in UNREACHED), "UNREACHED holds the two dead x6 instances only"
    stale = sorted(set(UNREACHED) & got)
    assert not stale, f"UNREACHED lists instances the grid search does reach: {stale}"
    assert set(UNREACHED) <= inst, f"UNREACHED lists instances the source does not have: {sorted(set(UNREACHED) - inst)}"
    # ... and the table reaches every instance the grid reaches
    table = set()
    for m in T.OPTION_SETS.values():
        for s in T.CASES:
            k = conv_key(s, m)
            table.add(("x6",) + k[1:5] if k[0] == 0 else ("lean", m, k[7], k[8]))
    assert got <= table, f"reached on the grid but by no case: {sorted(got - table)}"


def test_variant_cases_are_ragged_and_cover_the_edges():
    from buctd_amd import _C
    out = (C.c_int * 11)()
    for s in T.VARIANT_CASES:
        assert _C.lib().buctd_conv3x3_bf16x6_plan(*s, -1, out) == 0
        N, H, W, Ci, Co = s
        assert (N * H * W) % out[9] != 0 and (N * (H + 1) * (W + 1) + W + 1) % out[9] != 0, f"{s}: position tiles are not ragged"
    assert any(s[2] == 1 for s in T.VARIANT_CASES) and any(s[1] == 1 for s in T.VARIANT_CASES)
    assert any(s[2] == 74 for s in T.VARIANT_CASES), "W = MAX_SW - 1"
    assert any(s[3] > s[4] for s in T.VARIANT_CASES) and any(s[3] < s[4] for s in T.VARIANT_CASES)
