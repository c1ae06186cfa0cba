"""Closure of the bf16x6 GEMM case table (tests/helpers/gemm_x6_cases.py) over the launch forms of gemm_x6.hip (host only:
buctd_x6_gemm_plan runs the function that fills the launch of buctd_x6_gemm, buctd_x6_gemm_tile is the remap function
x6_gemm_kernel calls, buctd_x6_image_path the load-path predicate x6_image_kernel calls - none launches anything).

Every (row_major, branch of the XCD remap), every load form of the image kernel in both roles and every epilogue form that
occurs on the search grid must be reached by a case of the table, or be listed in UNREACHED with the reason.  The remap is
proved a bijection from linear workgroup ids onto tiles for every grid of the table and every grid up to 12 x 12, in both
orders: a dropped or doubled tile fails here without a GPU."""
import ctypes as C
import itertools

import pytest

from tests.helpers import gemm_x6_cases as T

# forms that the grid finds and no case reaches, and why.  The only place where forms are left out.
UNREACHED = {}

EINVAL = -1
ORDER_FORMS = {(rm, br) for rm in (0, 1) for br in ("total < 8", "rem == 0", "xcd < rem and xcd >= rem, per > 0")}
IMAGE_FORMS = {(role, f) for role in (0, 1) for f in ("vector", "gather: k groups", "gather: k stride",
                                                      "gather: K tail inside a group of 8", "gather: address not on 16 bytes",
                                                      "rows alternate")}


def table_plans():
    return [(c, T.plan(c.M, c.N, c.K)) for c in T.CASES]


def case_forms(c, pl):
    return ({("order",) + T.order_key(pl)} | {("image",) + f for f in T.image_forms(c.a, c.M, c.K, 0) | T.image_forms(c.b, c.N, c.K, 1)} |
            {("epilogue",) + f for f in T.epi_forms(c)})


@pytest.fixture(scope="module")
def table_forms():
    forms = set()
    for c, pl in table_plans():
        forms |= case_forms(c, pl)
    return forms


def test_the_plan_query_reports_the_launch_the_table_names():
    ids = [T.case_id(c) for c in T.CASES]
    assert len(set(ids)) == len(ids), "case ids repeat"
    for c, pl in table_plans():
        name = T.case_id(c)
        assert pl is not None, f"{name}: the launch would refuse the case"
        assert (pl["gx"], pl["gy"]) == (-(-c.M // T.BM), -(-c.N // T.BN)), f"{name}: {pl}"
        assert pl["KB"] == -(-c.K // T.KPAD) * (T.KPAD // 32) and pl["chunks"] * 2 == pl["KB"] and pl["chunks"] % 4 == 0, f"{name}: {pl}"
        assert pl["total"] == pl["gx"] * pl["gy"] and (pl["per"], pl["rem"]) == divmod(pl["total"], 8), f"{name}: {pl}"
        assert pl["row_major"] == int(pl["gx"] * T.BM > pl["gy"] * T.BN), f"{name}: {pl}"
        if c.grid is not None:
            assert (pl["gx"], pl["gy"], pl["row_major"]) == c.grid, f"{name}: {pl}"
        for role, V in ((0, c.M), (1, c.N)):
            vp, kp = T.image_dims(V, c.K, role)
            assert (vp, kp) == (-(-V // (T.BM, T.BN)[role]) * (T.BM, T.BN)[role], pl["KB"] * 32), name
    # the grids the issue names, by workgroups, shape and order
    grids = {c.grid for c in T.GRID_CASES}
    assert {(1, 1, 0), (3, 1, 1), (4, 2, 1), (5, 3, 1), (3, 5, 0), (9, 6, 0), (6, 9, 0)} <= grids
    assert any(g[0] * g[1] == 54 and g[2] == 1 for g in grids), "54 workgroups in row-major order"
    assert all(any(g[0] * g[1] > 8 and g[0] * g[1] % 8 == 0 and g[2] == rm for g in grids) for rm in (0, 1))
    assert {(c.M, c.N) for c in T.GRID_CASES} >= {(512, 384), (640, 576), (384, 960), (1152, 1152), (768, 1728)}
    assert all(c.K == 8 for c in T.GRID_CASES)
    # tails
    assert {1, 15, 16, 17, 127, 129, 191, 193} <= {c.M for c in T.TAIL_CASES} and {1, 15, 16, 17, 127, 129, 191, 193} <= {c.N for c in T.TAIL_CASES}
    assert any((c.M, c.N, c.K) == (1, 1, 1) for c in T.TAIL_CASES)
    assert {1, 7, 8, 9, 31, 33, 255, 256, 257, 513} <= {c.K for c in T.TAIL_CASES if c.a.ks == 1 and c.b.ks == 1}
    assert {T.plan(33, 20, K)["chunks"] for K in (256, 257, 513)} == {4, 8, 12}
    # address functions in both roles, epilogues, the fc_o layouts
    for ad in ("a", "b"):
        got = [getattr(c, ad) for c in T.ADDR_CASES]
        assert {1, 2, 3, 4} <= {x.off for x in got if x.ks == 1 and not x.kg} and {12, 20, 48} <= {x.vg for x in got} and {12, 20, 48} <= {x.kg for x in got}
        assert any(x.vs % 2 and x.ks == 1 and not x.vg for x in got) and any(x.vs == 1 and x.ks > 1 and not x.vg for x in got)
    assert all(T.AM % g and T.AN % g and T.AK % g and 8 % g and 16 % g for g in (12, 20, 48))
    assert {(c.N % 16 == 0) for c in T.FC_O_CASES} == {True, False} and len(T.FC_O_CASES) == 6
    assert {c.group for c in T.CASES} == set(T.GROUPS) and any(c.hard for c in T.CASES)
    assert all(c.M * c.N * c.K <= 1152 * 1152 * 8 for c in T.CASES)


def test_every_order_and_remap_branch_on_the_grid_has_a_case(table_forms):
    found = {}
    for M, N, K in itertools.product(T.GRID_M, T.GRID_N, T.GRID_K):
        pl = T.plan(M, N, K)
        assert pl is not None
        found.setdefault(T.order_key(pl), (M, N, K, pl))
    assert set(found) == ORDER_FORMS, f"grid: missing {sorted(ORDER_FORMS - set(found))}, unexpected {sorted(set(found) - ORDER_FORMS)}"
    have = {f[1:] for f in table_forms if f[0] == "order"}
    missing = [f"(row_major, remap branch) = {k}, e.g. {v[0]}x{v[1]}x{v[2]}: {v[3]}" for k, v in sorted(found.items())
               if k not in have and ("order",) + k not in UNREACHED]
    assert not missing, "workgroup orders without a case in tests/helpers/gemm_x6_cases.py:\n" + "\n".join(missing)
    # both branches of the ragged remap with more than one tile per XCD, in both orders
    for rm in (0, 1):
        assert any(pl["row_major"] == rm and pl["per"] > 1 and pl["rem"] for _, pl in table_plans()), f"row_major {rm}: per > 1 with rem != 0"


def test_every_image_load_form_on_the_grid_has_a_case(table_forms):
    found = {}
    n = 0
    for role, V, K, (name, f), off in itertools.product((0, 1), T.GRID_V, T.GRID_K, T.GRID_ADDR, T.GRID_OFF):
        n += 1
        for form in T.image_forms(f(V, K, off), V, K, role):
            found.setdefault(form, (name, V, K, off))
    assert n == 2 * 2 * 7 * 5 * 5
    assert set(found) == IMAGE_FORMS, f"grid: missing {sorted(IMAGE_FORMS - set(found))}, unexpected {sorted(set(found) - IMAGE_FORMS)}"
    have = {f[1:] for f in table_forms if f[0] == "image"}
    missing = [f"(role, load form) = {k}, e.g. {v[0]} {v[1]}x{v[2]} off {v[3]}" for k, v in sorted(found.items())
               if k not in have and ("image",) + k not in UNREACHED]
    assert not missing, "image load forms without a case in tests/helpers/gemm_x6_cases.py:\n" + "\n".join(missing)


def test_every_epilogue_form_has_a_case(table_forms):
    have = {f[1:] for f in table_forms if f[0] == "epilogue"}
    missing = sorted(k for k in T.EPI_FORMS if k not in have and ("epilogue",) + k not in UNREACHED)
    assert not missing, f"epilogue forms without a case: {missing}"
    assert any(c.epi.Nc and c.N % c.epi.Nc and c.N % 16 and c.epi.ldc > c.epi.Nc and c.epi.c_off for c in T.CASES)


def test_unreached_is_current(table_forms):
    assert not set(UNREACHED) & table_forms, "UNREACHED is stale"
    assert set(UNREACHED) <= ({("order",) + k for k in ORDER_FORMS} | {("image",) + k for k in IMAGE_FORMS} |
                              {("epilogue",) + k for k in T.EPI_FORMS})


def grids_to_prove():
    table = {(pl["gx"], pl["gy"]) for _, pl in table_plans()}
    return sorted(table | set(itertools.product(range(1, 13), range(1, 13))))


def test_the_remap_is_a_bijection_onto_the_tiles_in_both_orders():
    grids = grids_to_prove()
    assert {(18, 3), (9, 6), (6, 9), (5, 3), (3, 5), (4, 2), (3, 1), (1, 1)} <= set(grids)
    for (gx, gy), rm in itertools.product(grids, (0, 1)):
        tiles = [T.tile_of(lin, gx, gy, rm) for lin in range(gx * gy)]
        assert all(0 <= bx < gx and 0 <= by < gy for bx, by in tiles), f"{gx} x {gy} row_major {rm}: a tile outside the grid"
        assert len(set(tiles)) == gx * gy, (f"{gx} x {gy} row_major {rm}: {gx * gy - len(set(tiles))} tiles dropped, doubled: "
                                            f"{sorted(t for t in set(tiles) if tiles.count(t) > 1)[:4]}")


def test_the_workgroups_of_an_xcd_walk_one_operand_back_to_back():
    """the point of the order: the tiles an XCD (lin & 7) takes one after another are consecutive in the stated order, so
    row_major shares the row tile (the A blocks) and column-major the column tile"""
    for (gx, gy), rm in itertools.product(((5, 3), (3, 5), (9, 6), (18, 3), (4, 4), (3, 1)), (0, 1)):
        total = gx * gy
        for xcd in range(min(8, total)):
            seq = [T.tile_of(lin, gx, gy, rm) for lin in range(xcd, total, 8)]
            L = [bx * gy + by if rm else by * gx + bx for bx, by in seq]
            assert L == list(range(L[0], L[0] + len(L))), f"{gx} x {gy} row_major {rm} xcd {xcd}: {seq}"


def test_the_vector_loads_follow_the_address_not_the_offset():
    """an image source that is not on a 16-byte boundary gathers (16-byte loads need the alignment); every source that is takes
    the two 16-byte loads exactly where the element offset is a multiple of 4 - what the kernel did before for every caller"""
    V, K = 33, 52
    for role in (0, 1):
        for off in range(9):
            got = T.image_paths(T.contig(V, K, off), V, K, role)
            for (v, k0), vec in got.items():
                assert vec == int(k0 + 8 <= K and (off + v * K + k0) % 4 == 0), (role, off, v, k0)
        assert not any(T.image_paths(T.contig(V, K, 1), V, K, role).values())
        assert not any(T.image_paths(T.contig(V, K), V, K, role, base=T.BASE + 4).values())
        # the base and the offset add up: 12 bytes + 1 element is aligned again
        assert T.image_paths(T.contig(V, K, 1), V, K, role, base=T.BASE + 12) == T.image_paths(T.contig(V, K), V, K, role)
        # neither a k stride nor k groups ever take them
        assert not any(T.image_paths(T.transposed(V, K), V, K, role).values())
        assert not any(T.image_paths(T.kgrouped(V, K, 12), V, K, role).values())


def test_queries_and_launches_refuse_the_same_arguments():
    from buctd_amd import _C
    lib = _C.lib()
    out = (C.c_int * 8)()
    bx, by, vec = C.c_int(), C.c_int(), C.c_int(7)
    for M, N, K in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert lib.buctd_x6_gemm_plan(M, N, K, out) == EINVAL and list(out) == [0] * 8
        # the pointers are never dereferenced: the call returns before a launch
        assert lib.buctd_x6_gemm(M, N, K, T.BASE, T.BASE, None, 0, 1.0, T.BASE, 4, 0, 0, None) == EINVAL
        assert b"buctd_x6_gemm" in lib.buctd_last_error()
    assert lib.buctd_x6_gemm_plan(4, 4, 4, None) == EINVAL
    for lin, gx, gy, rm in ((-1, 2, 2, 0), (4, 2, 2, 0), (0, 0, 2, 0), (0, 2, 0, 1), (0, 2, 2, 2)):
        assert lib.buctd_x6_gemm_tile(lin, gx, gy, rm, C.byref(bx), C.byref(by)) == EINVAL
    assert lib.buctd_x6_gemm_tile(0, 2, 2, 0, None, C.byref(by)) == EINVAL
    good = (T.BASE, 20, 40, 0, 0, 40, 0, 0, 1, 0)
    assert lib.buctd_x6_image_path(*good, 3, 8, C.byref(vec)) == 0 and vec.value == 1
    for bad in ((None,) + good[1:], good[:1] + (0,) + good[2:], good[:2] + (0,) + good[3:], good[:9] + (2,), good[:3] + (-1,) + good[4:]):
        assert lib.buctd_x6_image_path(*bad, 3, 8, C.byref(vec)) == EINVAL and vec.value == 0
        if bad[0] is not None:
            assert lib.buctd_x6_image(*bad, T.BASE, None) == EINVAL
    for v, k0 in ((-1, 0), (20, 0), (0, -8), (0, 4), (0, 256)):
        assert lib.buctd_x6_image_path(*good, v, k0, C.byref(vec)) == EINVAL
    assert lib.buctd_x6_image_path(*good, 0, 248, C.byref(vec)) == 0 and vec.value == 0       # inside Kpad, past K
    assert lib.buctd_x6_image_path(*good, 3, 8, None) == EINVAL
