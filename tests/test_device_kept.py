"""The tables a roster keeps on the device between calls, through every subset of them that a call can pass.

A roster call passes a kept table -- the speaker state, the AFK messages, the room table, the users' descriptions, the who
table, the clone records, the relay's room names, the go table -- only when it changed.  The call uploads what it passes between the
roster's table and its own inputs, its kernel reads the uploads, and a tail of extra blocks copies them into the kept
allocations; a table that is not passed is read from its kept allocation (fanout.hip: ``pass_kept`` on the host,
``copy_kept`` in the kernels).  The other device modules pass subsets as their fuzzing happens to; this one passes every
subset of every call kind, 56 in all, on the smallest roster at which the copy tail can go wrong (65 slots, 3 look rooms,
3 clone records: table boundaries inside a block, more than one block, a partial last block).

Seven kinds make the same call twice and compare the arrays byte for byte: 40 cases.  ``go_many`` cannot: a call that moves
cannot be made twice, and one that moves nobody shows neither the phrases nor the clone records.  Its 16 cases are two
rounds each of two different calls that both walk (``run_go`` of the child): the first call's kernel reads the uploads, the
second's the kept allocations, and both are compared with the model's ``go_call`` and with a fresh roster seated in the
state each call met.

Host tier (unmarked): the cases are the 56 of the kinds' tables, and the tables have the sizes the copy tail is told.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_kept_child.py, under ``timeout``), and the tests assert on its JSON.  No number here is measured: the copy
volumes are sums of 256-byte aligned slices of arrays whose sizes the module's mirrors give.
"""
from __future__ import annotations

import json

import pytest

import child_run
from device_kept_child import CAPACITY, TABLES, TWICE, State, go_walks, input_arrays, new_roster, passed, request, subsets, table_slices

#: the kinds whose cases are one call made twice; go_many's have tests of their own below
KINDS = TWICE


def slice_of(n: int) -> int:
    """An array's 256-byte aligned slice of an upload (Carver of fanout.hip)."""
    return -(-n // 256) * 256


# ------------------------------------------------------------------ host tier
def test_the_cases_are_every_subset_of_every_kind():
    assert {k: len(subsets(t)) for k, t in TABLES.items()} == {"speak_many": 2, "input_many": 2, "tell_many": 4, "look_many": 8,
                                                              "who_many": 16, "rooms_many": 4, "relay_many": 4, "go_many": 16}
    assert sum(len(subsets(t)) for t in TABLES.values()) == 56 and sum(len(subsets(TABLES[k])) for k in KINDS) == 40
    assert TABLES["go_many"] == ("speech", "clones", "rooms", "go") and KINDS == tuple(TABLES)[:7]
    assert subsets(("a", "b")) == [(), ("a",), ("b",), ("a", "b")]


def test_the_tables_have_the_sizes_the_copy_tail_is_told():
    roster = new_roster(State("relay_many"))
    words = {t: sum(slice_of(n) if len(arrays) > 1 else n for n in arrays) // 4 for t, arrays in table_slices(roster).items()}
    assert words == {"speech": 260, "afk": 1040, "rooms": 804, "udesc": 520, "who": 130, "names": 18, "clones": 192, "go": 1430}
    # the boundaries fall inside a block, the who table and the names are shorter than one, and every tail but theirs ends in a
    # partial block
    assert all(w % 256 for w in words.values()) and words["who"] < 256 and words["names"] < 256 and CAPACITY == 65


def test_the_walks_of_a_go_case_swap_the_ends_and_come_back():
    """Without a device: a round's two calls are one move each, slot 0's and slot 64's, between the rooms at both ends."""
    st = State("go_many")
    assert go_walks(st) == [[(64, b"attic", 2), (0, b" attic now", 3)], [(0, b"attic", 2), (64, b"hall", 2)]]
    st.users[0]["room"], st.users[64]["room"] = 2, 0
    assert go_walks(st) == [[(0, b"attic", 2), (64, b" attic now", 3)], [(64, b"attic", 2), (0, b"hall", 2)]]


@pytest.mark.parametrize("kind", tuple(TABLES))
def test_a_change_sets_the_flag_of_its_table_alone(kind):
    """Without a device: after the flags are cleared as a call clears them, every subset's changes set exactly its flags."""
    st = State(kind)
    roster = new_roster(st)
    for subset in subsets(TABLES[kind]):
        for f in ("_dirty", "_speech_dirty", "_private_dirty", "_afk_dirty", "_rooms_dirty", "_udesc_dirty", "_who_dirty", "_clones_dirty",
                  "_go_dirty"):
            setattr(roster, f, False)
        if kind == "relay_many":
            roster._relay_names = roster._prepare_relay(request(kind, st), None, None)[2]
        for table in subset:
            st.change(roster, table)
        assert passed(kind, roster, request(kind, st)) == list(subset) and not roster._dirty
        assert all(n >= 0 for n in input_arrays(kind, request(kind, st), st))


# ------------------------------------------------------------------ GPU tier
@pytest.fixture(scope="module")
def kept_run(built):
    res = child_run.run_child("device_kept_child.py", "DEVICE_KEPT", 120)
    print("\n[kept]", json.dumps(res)[:4000])
    return res


def cases_of(run, kind):
    cases = [c for c in run["cases"] if c["kind"] == kind]
    assert [tuple(c["subset"]) for c in cases] == subsets(TABLES[kind])
    return cases


@pytest.mark.gpu
def test_every_subset_of_every_kind_ran(kept_run):
    assert len(kept_run["cases"]) == 56 and kept_run["order"] == {k: list(v) for k, v in TABLES.items()}
    assert len([c for c in kept_run["cases"] if c["kind"] != "go_many"]) == 40


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_exactly_the_changed_tables_are_passed(kept_run, kind):
    for c in cases_of(kept_run, kind):
        assert c["flags"] == c["subset"] and not c["table_dirty"] and c["flags_after"] == [], c


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_the_uploads_and_the_kept_tables_read_alike(kept_run, kind):
    """Call 1 read the uploads, call 2 the kept allocations its copy tail filled: the same bytes in every output array, and
    through the accessors what a fresh roster in the final state returns, and what the CPU models say."""
    for c in cases_of(kept_run, kind):
        assert c["arrays"] >= 5 and c["arrays_differ"] == [], c
        assert c["again_says_the_same"] and c["fresh_says_the_same"], c
        assert c["model_differences"] == [[], []], c


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_the_first_passed_table_and_all_behind_it_travel(kept_run, kind):
    """upload() copies from the first passed table to the end of the inputs: the clean figure is the inputs' slices and the
    violation count, and call 1 adds the slices from the first passed table through the last table of the layout.  The
    roster's table is resident: no slice of it in either."""
    order = list(TABLES[kind])
    for c in cases_of(kept_run, kind):
        clean = sum(slice_of(n) for n in c["inputs"]) + 4
        behind = order[min(order.index(t) for t in c["subset"]):] if c["subset"] else []
        assert c["h2d"][1] == clean, c
        assert c["h2d"][0] - clean == sum(slice_of(n) for t in behind for n in c["tables"][t]), c
        assert c["d2h"][0] == c["d2h"][1], c


# ------------------------------------------------------------------ go_many: two rounds of two different calls
def go_rounds(run):
    cases = cases_of(run, "go_many")
    assert len(cases) == 16 and all(len(c["rounds"]) == 2 and all(len(r["calls"]) == 2 for r in c["rounds"]) for c in cases)
    return [(c, r) for c in cases for r in c["rounds"]]


@pytest.mark.gpu
def test_go_many_passes_exactly_the_changed_tables_and_its_moves_leave_nothing_dirty(kept_run):
    """The flags before a round's first call are exactly the subset, the table clean; after it none remain, the table's
    included, because the look inside the call uploaded it; and the second call leaves none either."""
    for c, r in go_rounds(kept_run):
        assert r["flags"] == c["subset"], c
        assert [call["flags_after"] for call in r["calls"]] == [[], []], c


@pytest.mark.gpu
def test_go_many_reads_the_uploads_and_the_kept_tables_as_the_model_does(kept_run):
    """Both calls of every round walk one of the two ends and keep the room it leaves private: the model's differences are
    empty, and a fresh roster seated in the state each call met says the same."""
    for c, r in go_rounds(kept_run):
        for call in r["calls"]:
            assert call["outcomes"] == [6, 0] and call["returned"] == [False, False], (c["subset"], call)        # already; walked
            assert call["model_differences"] == [] and call["fresh_says_the_same"], (c["subset"], call)
    # who stayed behind, and so the least that keeps the room private: three of a room's four users, then four of the five
    # that the first walk made; in the first round of a case that changes the clone records, a record beside them
    for c in cases_of(kept_run, "go_many"):
        at_the_ends = int("clones" in c["subset"])
        assert [[call["stay"] for call in r["calls"]] for r in c["rounds"]] == [[3 + at_the_ends, 4 + at_the_ends], [3, 4]], c["subset"]
    assert cases_of(kept_run, "go_many")[0]["primed"] == [True] * 4


@pytest.mark.gpu
def test_go_many_copies_from_the_first_passed_table_through_the_go_table(kept_run):
    """The first call's upload is the inputs' slices and the violation count, and the slices from the first passed table
    through the last of the layout; the second call's is the inputs' alone.  The look's own upload -- the table, after the
    move -- is the look's, not the call's."""
    order = list(TABLES["go_many"])
    for c, r in go_rounds(kept_run):
        first, second = r["calls"]
        behind = order[min(order.index(t) for t in c["subset"]):] if c["subset"] else []
        clean = [sum(slice_of(n) for n in call["inputs"]) + 4 for call in r["calls"]]
        assert second["h2d"] == clean[1], (c["subset"], second)
        assert first["h2d"] - clean[0] == sum(slice_of(n) for t in behind for n in c["tables"][t]), (c["subset"], first)
        assert first["look_h2d"] is not None and second["look_h2d"] is not None
