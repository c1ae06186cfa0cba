"""The case table of tests/helpers/grad_contract_cases.py against the source of buctd_amd/ops.py and ops_seq.py (no GPU):
every function that calls grad_target - the place where a node decides where a parameter gradient is written - is named in
the `sites` of at least one case, and the table names no function that does not exist.  A new node, or a new grad_target
call in a function no case claims, fails here; tests/test_gpu_grad_contract.py asserts that each case's backward really
passes through the sites it names."""
import textwrap

from tests.helpers import grad_contract_cases as G


def test_every_grad_target_site_is_named_by_a_case():
    sites = sorted(set(G.grad_target_calls().values()))
    claimed = {s for c in G.CASES for s in c["sites"]}
    print("\n" + "\n".join(f"  {s:32s} {[c['name'] for c in G.CASES if s in c['sites']][:3]}" for s in sites))
    assert len(sites) >= 9, f"the walk found only {sites}"
    missing = [s for s in sites if s not in claimed]
    assert not missing, f"no case of grad_contract_cases.CASES names {missing}"


def test_the_table_names_only_functions_that_exist_and_call_grad_target():
    have = G.functions_in_sources()
    callers = set(G.grad_target_calls().values())
    for c in G.CASES:
        assert c["sites"], c["name"]
        for s in c["sites"]:
            assert s in have, f"{c['name']}: {s} is no function of {G.SOURCES}"
            assert s in callers, f"{c['name']}: {s} does not call grad_target"


def test_case_names_are_unique_and_the_side_lists_name_cases():
    assert len(G.BY_NAME) == len(G.CASES)
    for name in G.MULTI_OUTPUT + G.MIXED_NORM:
        assert name in G.BY_NAME


def test_the_walk_sees_a_new_call_site(tmp_path):
    """a grad_target call added to a function that no case names is found by the walk"""
    src = textwrap.dedent('''
        class NewNode:
            @staticmethod
            def backward(ctx, dy):
                g, acc = ops.grad_target(ctx.w)
                return g

        def helper(p):
            return grad_target(p)

        def grad_target(p):
            return p, 0
    ''')
    (tmp_path / "new_ops.py").write_text(src)
    calls = G.grad_target_calls(("new_ops.py",), str(tmp_path))
    assert sorted(calls.values()) == ["NewNode.backward", "helper"]
    claimed = {s for c in G.CASES for s in c["sites"]}
    assert not set(calls.values()) & claimed
