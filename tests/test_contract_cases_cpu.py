"""The registry of tests/contract_cases.py against include/tsim.h, without a GPU: every entry point that takes a workspace is
named by a case the poison test runs, every entry point that takes a stream by a case the stream test runs — or is exempt with
a reason — so a new entry point fails here until it gets a case; the decoys satisfy their conditions on the oracles alone; and
the set of cases whose Python op reads back mid-call is pinned."""
import numpy as np
import pytest

import contract_cases as cases


def test_the_header_has_the_entries_the_registry_was_written_for():
    ws, st = cases.header_entries()
    assert len(ws) == len(set(ws)) and len(st) == len(set(st))
    assert set(ws) <= set(st), "an entry that takes a workspace takes a stream"
    assert (len(ws), len(st)) == (28, 57), (len(ws), len(st))
    assert "tsim_mst_prim" in ws and "tsim_l2norm_rows" in st and "tsim_l2norm_rows" not in ws


def test_every_workspace_entry_is_named_by_a_poison_case():
    ws, _ = cases.header_entries()
    named = {e for c in cases.WORKSPACE_CASES for e in c.entries}
    missing = [e for e in ws if e not in named and e not in cases.EXEMPT]
    assert not missing, f"entries with a workspace and no case in tests/contract_cases.py: {missing}"


def test_every_stream_entry_is_named_by_a_stream_case():
    _, st = cases.header_entries()
    named = {e for c in cases.CASES for e in c.entries}
    missing = [e for e in st if e not in named and e not in cases.EXEMPT]
    assert not missing, f"entries with a stream and no case in tests/contract_cases.py: {missing}"


def test_exemptions_are_real_entries_with_reasons_and_no_case():
    ws, st = cases.header_entries()
    named = {e for c in cases.CASES for e in c.entries}
    for e, why in cases.EXEMPT.items():
        assert e in st, f"{e} is not an entry with a stream parameter"
        assert e not in named, f"{e} has a case: drop its exemption"
        assert isinstance(why, str) and len(why.split()) >= 4 and "\n" not in why, e
    assert not set(ws) & set(cases.EXEMPT), "every entry that takes a workspace has its poison case"
    for c in cases.CASES:
        for e in c.entries:
            assert e in st, (c.name, e)
        assert (c.workspace is not None) == bool(set(c.entries) & set(ws)), c.name


def test_host_sync_cases_are_pinned():
    """An op that starts reading back from the device mid-call shows up here (and loses the stream test's side.query() check)."""
    assert cases.HOST_SYNC_CASES == ["community-detection", "hdbscan", "range-cosine-tau", "range-cosine-tau_q", "range-dot-tau", "range-dot-tau_q", "range-l2-tau",
                                     "range-l2-tau_q"]


@pytest.mark.parametrize("case", cases.CASES, ids=repr)
def test_operands_have_one_layout(case):
    """real, decoy and other operands have the same names, shapes and dtypes: one workspace layout, and a copy_ in place."""
    real = case.operands("real")
    for which in ("decoy", "other"):
        o = case.operands(which)
        assert list(o) == list(real), (which, list(o))
        for k in real:
            assert o[k].shape == real[k].shape and o[k].dtype == real[k].dtype, (which, k, o[k].shape, o[k].dtype)
    assert case.decoy_rule in ("beats", "looser", "other"), case.name


@pytest.mark.parametrize("case", [c for c in cases.CASES if c.decoy_check is not None], ids=repr)
def test_decoy_conditions_hold_on_the_oracles(case):
    real, decoy = case.oracle("real"), case.oracle("decoy")
    assert len(real) == len(decoy)
    case.decoy_check(real, decoy)
    other = case.oracle("other")
    assert not all(cases.same(a, b) for a, b in zip(real, other)), "the other operands give the real result"


def test_the_route_cases_keep_their_shapes():
    """The thresholds the two large cases exist for (csrc/k1_topk.h plan_prepass, csrc/search.hip plan_two_phase)."""
    q, c = cases.by_name("flat-prepass").operands("real").values()
    assert c.shape[0] >= 262144 and q.shape[0] <= 768
    q, c = cases.by_name("flat-two-phase").operands("real").values()
    assert c.shape[0] >= 4 * 131072 and q.shape[0] > 768
    for name in ("range-cosine-tau", "range-dot-tau", "range-l2-tau"):
        lims, _, _, st = cases.by_name(name).oracle("real")
        assert st[0] == 1 and st[1] == 2 and np.diff(lims)[1] > 2048, (name, st, np.diff(lims))
    st = cases.by_name("range-cosine-tau_q").oracle("real")[3]
    assert st[2] == 2 and np.diff(cases.by_name("range-cosine-tau_q").oracle("real")[0])[2] == cases.RANGE_N


def test_the_row_preselection_of_the_large_oracle_changes_nothing():
    """contract_cases._big_oracle hands oracle.search_ref.cosine_topk_f32 only the rows that can be in a query's top-k.  On one
    query of the pre-pass corpus, real and decoy (planted copies and near-ties: every score at the top is a tie or nearly one), the
    full cosine_topk_f32 over all 262 144 rows gives the same bits and the same rows."""
    case = cases.by_name("flat-prepass")
    for which in ("real", "decoy"):
        h = case.operands(which)
        s, i = cases.cosine_topk_f32(h["q"][:1], h["c"], cases.BIG_K)
        want = case.oracle(which)
        assert cases.same(s[0], want[0][0]) and cases.same(i[0], want[1][0]), which
