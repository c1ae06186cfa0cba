"""The case tables of tests/helpers/stream_cases.py against the code paths of the streaming kernels (no GPU): every path
name of every kernel is taken by a case, the long cases reach the loop trip they exist for, and no case needs more than
200 MB of operands and references."""
import pytest

from tests.helpers import stream_cases as S


@pytest.mark.parametrize("kernel", sorted(S.PATHS))
def test_every_path_is_taken_by_a_case(kernel):
    taken = {}
    for case in S.TABLES[kernel]:
        for name in S.path_of(kernel, case):
            assert name in S.PATHS[kernel], f"{kernel}: case {case} takes a path that PATHS does not list: {name}"
            taken.setdefault(name, case)
    print(f"\n{kernel}: {len(S.TABLES[kernel])} cases")
    for name in S.PATHS[kernel]:
        print(f"  {name:32s} {taken.get(name, '-')}")
    missing = [n for n in S.PATHS[kernel] if n not in taken]
    assert not missing, f"{kernel}: no case takes {missing}"


def test_tables_and_paths_name_the_same_kernels():
    assert sorted(S.TABLES) == sorted(S.PATHS)


@pytest.mark.parametrize("i", range(len(S.SECOND_TRIPS)))
def test_long_cases_reach_their_second_trip(i):
    kernel, pick, name = S.SECOND_TRIPS[i]
    cases = [c for c in S.TABLES[kernel] if pick(c)]
    assert cases, f"{kernel}: the table has no case for {name}"
    for c in cases:
        assert name in S.path_of(kernel, c), f"{kernel} {c} does not reach {name}"


def test_the_dispatch_thresholds_sit_between_neighbouring_cases():
    assert "softmax:wave" in S.path_of("softmax", (1, 512, 3.0)) and "softmax:block" in S.path_of("softmax", (1, 513, 3.0))
    assert S.stream_trips(4096 * 256) == 1 and S.stream_trips(4096 * 256 + 1) == 2
    assert S.colsum_chunk_rows(64 * 8192) == 64 and S.colsum_chunk_rows(64 * 8192 + 1) == 65
    assert S.bwd2_blocks(4100) == (65, 64) and S.bwd2_blocks(12 * 96 * 72) == (1024, 81)
    assert S._fin(2048) == "finalize:one-trip" and S._fin(2049) == "finalize:second-trip"
    assert S.bn_acc_ok(1024) and not S.bn_acc_ok(2048) and not S.bn_acc_ok(3)


def test_no_case_is_larger_than_200_mb():
    for kernel, table in S.TABLES.items():
        for case in table:
            assert S.case_bytes(kernel, case) < 200e6, f"{kernel} {case}: {S.case_bytes(kernel, case) / 1e6:.0f} MB"
