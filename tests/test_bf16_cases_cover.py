"""The case tables of tests/helpers/bf16_cases.py against the code paths of csrc/conv_bf16.hip (no GPU): every path name of
every kernel - all 18 bf16_conv_kernel<MT, NT, VEC> instances among them - is taken by a case, the long cases reach the loop
trip they exist for, the sizes stay within the stated limits, and the restated MT / NT rule agrees with the one
tests/test_gpu_bf16_inference.py asserts."""
import pytest

from tests.helpers import bf16_cases as B


@pytest.mark.parametrize("kernel", sorted(B.PATHS))
def test_every_path_is_taken_by_a_case(kernel):
    taken = {}
    for case in B.TABLES[kernel]:
        for name in B.path_of(kernel, case):
            assert name in B.PATHS[kernel], f"{kernel}: case {case} takes a path that PATHS does not list: {name}"
            taken.setdefault(name, case)
    print(f"\n{kernel}: {len(B.TABLES[kernel])} cases")
    for name in B.PATHS[kernel]:
        print(f"  {name:32s} {taken.get(name, '-')}")
    missing = [n for n in B.PATHS[kernel] if n not in taken]
    assert not missing, f"{kernel}: no case takes {missing}"


def test_tables_and_paths_name_the_same_kernels():
    assert sorted(B.TABLES) == sorted(B.PATHS)
    assert len([n for n in B.PATHS["conv"] if n.startswith("inst:")]) == 18


def test_each_large_conv_case_is_one_instance_with_a_large_tile():
    insts = [B.conv_instance(c) for c in B.CONV_LARGE]
    assert sorted(insts) == sorted((mt, nt, vec) for mt in (2, 4) for nt in (2, 3, 4) for vec in (True, False))
    assert all(B.conv_instance(c)[0] == 1 for c in B.CONV_SMALL)
    assert all(c[2] == c[0] // 2 for c in B.CONV_LARGE), "the existing GPU test runs these with pad = R // 2"


@pytest.mark.parametrize("i", range(len(B.SECOND_TRIPS)))
def test_long_cases_reach_their_second_trip(i):
    kernel, pick, name = B.SECOND_TRIPS[i]
    cases = [c for c in B.TABLES[kernel] if pick(c)]
    assert cases, f"{kernel}: the table has no case for {name}"
    for c in cases:
        assert name in B.path_of(kernel, c), f"{kernel} {c} does not reach {name}"


def test_the_dispatch_thresholds_sit_where_the_host_code_puts_them():
    # Co = 512: nN = 8, MT = 4 from M = 32,513, MT = 2 from 16,257; Co = 336: NT = 3, nN = 7; Co <= 32: nN = 1
    assert (B.conv_mt(32512, 512), B.conv_mt(32513, 512)) == (2, 4)
    assert (B.conv_mt(16256, 512), B.conv_mt(16257, 512)) == (1, 2)
    assert B.conv_nt(336) == 3 and (B.conv_mt(37376, 336), B.conv_mt(37377, 336)) == (2, 4)
    assert (B.conv_mt(18688, 336), B.conv_mt(18689, 336)) == (1, 2)
    assert (B.conv_mt(261888, 32), B.conv_mt(261889, 32)) == (2, 4) and (B.conv_mt(130944, 32), B.conv_mt(130945, 32)) == (1, 2)
    assert [B.conv_nt(c) for c in (1, 32, 33, 48, 64, 96, 144, 192, 256, 336, 384)] == [2, 2, 4, 3, 4, 3, 3, 4, 4, 3, 4]
    assert B.conv_vec(8) and B.conv_vec(384) and not B.conv_vec(3) and not B.conv_vec(44)
    assert B.image_k(3, 3) == 32 and B.image_k(8, 3) == 96 and B.image_k(32, 1) == 32 and B.image_k(384, 3) == 3456
    assert B.grid_trips(4096 * 256, 4096) == 1 and B.grid_trips(4096 * 256 + 1, 4096) == 2
    assert B.grid_trips(8192 * 256, 8192) == 1 and B.grid_trips(8192 * 256 + 1, 8192) == 2


def test_conv_cases_stay_small():
    for case in B.CONV + B.CONV_POISON:
        assert B.conv_macs(case) <= B.CONV_MAX_MACS, f"{case}: M * Co * Kt = {B.conv_macs(case):.3g}"
    for kernel, table in B.TABLES.items():
        for case in table:
            assert B.case_bytes(kernel, case) < B.CONV_MAX_BYTES, f"{kernel} {case}: {B.case_bytes(kernel, case) / 1e6:.0f} MB"


def test_poison_cases_have_k_padding():
    for case in B.CONV_POISON:
        assert "k:padded" in B.path_of("conv", case) and not case[8], case
    assert {B.conv_instance(c)[2] for c in B.CONV_POISON} == {True, False}


def test_integer_operands_are_exact_in_fp32():
    """the largest partial sum of the integer operands, Kt * 4 * 4 + 16 + 8, is an integer below 2^24"""
    for case in B.CONV:
        assert B.conv_geom(case)[3] * 16 + 24 < 1 << 24


# the workload shapes tests/test_gpu_bf16_inference.py used before the small cases: (R, stride, Ci, Co, N, H, W), MT
WORKLOAD_SHAPES = [((1, 1, 64, 256, 4, 128, 128), 4), ((3, 1, 32, 96, 1, 256, 256), 2), ((3, 2, 3, 64, 10, 384, 288), 4),
                   ((3, 2, 3, 64, 8, 384, 288), 2)]


def test_restated_tile_rule_agrees_with_the_existing_gpu_test():
    from tests.test_gpu_bf16_inference import LARGE_CASES, _tile_mt
    assert len(LARGE_CASES) == len(B.CONV_LARGE)
    for (R, stride, Ci, Co, N, H, W, *_), mt in [(c, m) for c, m, _ in LARGE_CASES] + WORKLOAD_SHAPES:
        M = N * B.conv_out(H, R, stride, R // 2) * B.conv_out(W, R, stride, R // 2)
        assert B.conv_mt(M, Co) == _tile_mt(M, Co) == mt, (R, stride, Ci, Co, N, H, W)
