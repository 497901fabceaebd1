"""CPU: the host side of the three beam searches (ctc_beam.hip, ctc_gram_decode.hip, asg_beam.hip) answers what it answered
before it was rewritten around one layout plan and one argument block -- every workspace / row / width query over a grid that
reaches each branch of the layouts, and, of a list of refused calls, the return code and the message: one argument error each,
and two at once, where the first error wins and so pins the order of an entry's checks.  The expected values were recorded from
a build of the parent commit by tests/golden/make_beam_abi_golden.py; the grid and the calls are tests/beam_abi_cases.py's."""
import json
import os

import numpy as np
import pytest

import beam_abi_cases as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    from end2end_amd import _lib
    return _lib.load(), _lib


def test_every_query_answers_what_the_parent_answered(lib):
    L, _ = lib
    want = np.load(os.path.join(GOLDEN, "beam_queries_parent.npz"))
    grid, got = A.query_grid(), A.run_queries(L)
    assert sorted(grid) == sorted({k.split("/")[0] for k in want.files})
    points = 0
    for name, rows in grid.items():
        assert np.array_equal(np.array(rows, dtype=np.int32), want[name + "/args"]), name       # the grid the values were recorded on
        g, w = np.array(got[name], dtype=np.int64), want[name + "/values"]
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (name, [(rows[i], int(g[i]), int(w[i])) for i in bad[:5]], bad.size)
        points += len(rows)
    # the CTC grid: 1680 points and the five that must give 0; the cut queries at five or six distinct cutoff_top_n each
    assert len(grid["e2e_ctc_beam_nbest_workspace_bytes"]) == 1685 and len(grid["e2e_ctc_beam_cut_workspace_bytes"]) >= 5 * 1685
    assert points > 30000


def test_the_grid_reaches_every_branch_of_the_ctc_layouts(lib):
    L, _ = lib
    general = {(V, W, lm) for V in A.CTC_V for W in A.CTC_W for lm in (0, 1) if L.e2e_ctc_beam_stream_workspace_bytes(1, V, W, lm)}
    fits = {(V, W, lm) for V in A.CTC_V for W in A.CTC_W for lm in (0, 1) if L.e2e_ctc_beam_stream_row_bytes(40, V, W, lm, 0)}
    assert general and fits - general and {(V, 513, lm) for V in A.CTC_V for lm in (0, 1)}.isdisjoint(fits)     # both kernels, and neither
    assert any(L.e2e_ctc_beam_workspace_bytes_lm(3, 40, V, W, 1) > L.e2e_ctc_beam_workspace_bytes_lm(3, 40, V, W, 0) for V, W, _ in general)
    # cutoff_top_n >= V: the query is the larger of the pruned and the plain one, and each of the two is the larger somewhere
    wins = set()
    for V, W, lm in fits:
        pruned_small = L.e2e_ctc_beam_cut_workspace_bytes(3, 40, V, W, lm, 1, 1)
        both = L.e2e_ctc_beam_cut_workspace_bytes(3, 40, V, W, lm, 1, V)
        plain = L.e2e_ctc_beam_nbest_workspace_bytes(3, 40, V, W, lm, 1)
        assert both >= plain and pruned_small > 0
        wins.add(both == plain)
    assert wins == {False, True}


def test_refused_calls_report_what_the_parent_reported(lib):
    L, L_mod = lib
    with open(os.path.join(GOLDEN, "beam_refused_parent.json")) as f:
        want = json.load(f)
    got = A.run_refused(L, L_mod)
    assert sorted(got) == sorted(want)
    wrong = {cid: (got[cid], want[cid]) for cid in got if got[cid] != want[cid]}
    assert not wrong, (len(wrong), dict(list(wrong.items())[:5]))


def test_the_refused_calls_cover_every_entry_with_two_errors_at_once():
    cases = A.refused_calls()
    entries = [e for fam, _, _ in A.FAMILIES for e in fam]
    assert {"e2e_ctc_beam", "e2e_ctc_beam_nbest", "e2e_ctc_beam_nbest_opt", "e2e_ctc_beam_nbest_cut", "e2e_ctc_beam_stream",
            "e2e_ctc_beam_stream_cut", "e2e_gram_ctc_beam_nbest", "e2e_gram_ctc_beam_nbest_opt", "e2e_gram_ctc_beam_stream",
            "e2e_asg_beam_nbest", "e2e_asg_beam_nbest_opt", "e2e_asg_beam_stream"} <= set(entries)
    for fam, _, _ in A.FAMILIES:
        for entry, (_, steps) in fam.items():
            names = [n for n, _ in steps]
            pairs = {cid.split("/")[1] for cid, _, e, _ in cases if e == entry and "+" in cid}
            assert len(pairs) >= 10, (entry, len(pairs))
            assert {"%s+%s" % p for p in zip(names, names[1:])} <= pairs, entry       # every adjacent pair of the entry's order
    for entry in ("e2e_ctc_beam_nbest_cut", "e2e_ctc_beam_stream_cut"):
        assert "%s/cutoff_prob+blank" % entry in {cid for cid, _, _, _ in cases}


def test_each_step_trips_its_own_check_and_the_steps_are_in_the_parents_order():
    """From the recorded messages: a step alone reports its own error (so its change does trip the check it is named for), and
    two steps together report the earlier one's (so the order the steps are listed in is the order the parent made its checks
    in; a step's change trips its check whatever the other step changes, tests/beam_abi_cases.py)."""
    with open(os.path.join(GOLDEN, "beam_refused_parent.json")) as f:
        want = json.load(f)
    for fam, _, _ in A.FAMILIES:
        for entry, (_, steps) in fam.items():
            for name, _ in steps:
                assert A.EXPECT[name] in want["%s/%s" % (entry, name)][1], (entry, name, want["%s/%s" % (entry, name)])
    for cid, (rc, msg) in want.items():
        case = cid.split("/")[1]
        if "+" in case:
            first, second = case.split("+")
            assert A.EXPECT[first] in msg, (cid, msg)
