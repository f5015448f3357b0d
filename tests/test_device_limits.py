"""Every call of ``device.Roster`` at the sizes the API accepts: 65,536 slots (``MAX_CAPACITY``), 1,024 look rooms, 1,024
review rooms, 65,536 clone records, revtell rings -- the accept side of the guards that the other device modules only
show to refuse.

Host tier (unmarked): the one statement this module adds to the models, ``admits_np``, equals ``nuts_path.admits`` over
the full truth table, and ``admit_words`` equals it over ``Roster.table``; the limits are accepted together; and the
coverage conditions, from the models alone -- the planted slots, rooms and records are present and distinct, the footer
counts of the full roster have five digits, every tell case resolves to the branch it is named for, some who line has a
``colour_com_count`` of 19, some relay happens at record 65,535, ring 1,023 and revtell ring 65,535 are non-empty.  A
planted input that is not the edge it was planted for would let the GPU tier pass for the wrong reason.  The helpers of
the binding whose loops only turn at tens of megabytes (``_gather``, ``_offsets``, ``_unpack``) are run with a small step
and past 2^31 here.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_limits_child.py, under ``timeout``), and the tests assert on its JSON: no difference from the models in
any part, a positive number of comparisons in every part, and the coverage conditions again on the device's answers.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import child_run
import device_limits_child as limits
from device_limits_child import (CAPACITY, EDGE_CLONES, EDGE_ROOMS, EDGE_SLOTS, FULL_LOOKERS, FULL_WHO_LOOKERS, GUARD_K, GUARD_LINES, LAST,
                                 LAST_ROOM, admit_words, admits_np, edge_coverage, edge_description, edge_script, footer_counts,
                                 full_description, full_renames, full_tell_cases)
from device_look_child import members
from device_tell_child import private
from device_who_child import colour_com_count, listed, shown
from nuts333_amd import device, nuts_path

CALLS = ("plan_many", "broadcast_many", "expand", "speak_many", "input_many", "review_many", "tell_many", "revtell_many", "look_many",
         "who_many", "relay_many")


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded by a host-tier test")
    monkeypatch.setattr(device, "_load", refuse)


@pytest.fixture(scope="module")
def full():
    return full_description()


@pytest.fixture(scope="module")
def edge():
    return edge_coverage()


# ------------------------------------------------------------------ host tier: the predicate over arrays
def test_the_numpy_predicate_is_np_fanout_admits_over_its_full_truth_table(built):
    """All 2^6 listener states x rm_is_null x force_listen x {SAY, SHOUT, SEMOTE}: the 768 cases of test_device_fanout.py."""
    states = np.array([[(s >> k) & 1 for k in range(6)] for s in range(64)], dtype=bool)
    cases = 0
    for rm_is_null in (0, 1):
        for force_listen in (0, 1):
            for com in (device.COM_SAY, device.COM_SHOUT, device.COM_SEMOTE):
                got = admits_np(*states.T, bool(rm_is_null), bool(force_listen), np.int64(com))
                want = [nuts_path.admits([int(x) for x in st], rm_is_null, force_listen, com) for st in states]
                assert got.tolist() == want, (rm_is_null, force_listen, com)
                cases += len(want)
    assert cases == 64 * 2 * 2 * 3 == 768


def test_admit_words_is_the_predicate_over_the_rosters_table(built, no_library):
    """The listener fields derived from the mirrors as ``Roster.table`` derives them, at a capacity that is no multiple of
    64, packed as a Plan packs them."""
    cap = 200
    rng = np.random.default_rng(5)
    r = device.Roster(cap)
    r.update(list(range(cap)), room=[None if x == 3 else int(x) for x in rng.integers(0, 4, cap)], login=(rng.random(cap) < 0.2).tolist(),
             ignall=(rng.random(cap) < 0.3).tolist(), ignshout=(rng.random(cap) < 0.3).tolist(), colour=(rng.random(cap) < 0.5).tolist())
    bs = [(b"", rm, sender, fl, com) for rm in (0, 2, 7, None) for sender in (None, 0, 199) for fl in (0, 1)
          for com in (device.COM_SAY, device.COM_SHOUT, device.COM_EMOTE, device.COM_SEMOTE)]
    got = admit_words(r._room, r._flags, bs, step=7)
    assert got.shape == (len(bs), 4) and got.dtype == np.uint64
    for k, (_, rm, sender, fl, com) in enumerate(bs):
        want = np.array([nuts_path.admits(row[:6].tolist(), int(rm is None), fl, com) for row in r.table(rm, sender)])
        assert got[k].tolist() == device._pack(want).tolist(), bs[k]


# ------------------------------------------------------------------ host tier: the limits, and the binding's helpers
def test_the_limits_are_accepted_together(no_library):
    assert (device.MAX_CAPACITY, device.MAX_LOOK_ROOMS, device.MAX_REVIEW_ROOMS) == (65536, 1024, 1024) == (CAPACITY, LAST_ROOM + 1, 1024)
    r = device.Roster(device.MAX_CAPACITY, look_rooms=device.MAX_LOOK_ROOMS, review_rooms=device.MAX_REVIEW_ROOMS, revtell=True,
                      clones=device.MAX_CAPACITY)
    assert (r.capacity, r.look_rooms, r.review_rooms, r.revtell, r.clones) == (65536, 1024, 1024, True, 65536)
    for kw in ({"look_rooms": 1025}, {"review_rooms": 1025}, {"clones": 65537}):
        with pytest.raises(ValueError):
            device.Roster(device.MAX_CAPACITY, **kw)
    with pytest.raises(ValueError):
        device.Roster(device.MAX_CAPACITY + 1)


def test_the_guard_plan_lies_on_the_accept_side(no_library):
    """4,096 broadcasts to 65,536 slots: 2^28 cells, 2^22 bitmap words, far below the guards of ``_checked``."""
    assert GUARD_K * CAPACITY >= 2**28 and GUARD_K * (CAPACITY // 64) < 2**31 and len(set(GUARD_LINES)) == 10
    r = device.Roster(CAPACITY)
    bs = [(GUARD_LINES[k % 10], k % 3, LAST, 0, device.COM_SAY) for k in range(GUARD_K)]
    packed = r._prepare_plan(bs)
    assert len(packed[2]) == GUARD_K and packed[4].max() == LAST
    with pytest.raises(ValueError, match="must be below 2\\^31"):
        r._checked([()] * 2**21, 1024, "K x ceil(capacity / 64)")


def test_gather_in_many_steps_is_the_concatenation(no_library):
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, 5000, dtype=np.uint8)
    counts = rng.integers(0, 40, 700)
    counts[[0, 5, 699]] = 0
    starts = rng.integers(0, len(src) - 40, 700)
    want = np.concatenate([src[s:s + n] for s, n in zip(starts, counts)])
    for step in (1, 7, 64, 1000, 1 << 24):
        assert np.array_equal(device._gather(src, starts, counts, step=step), want), step
    assert len(device._gather(src, starts[:0], counts[:0])) == 0
    one = device._gather(src, np.array([10]), np.array([4000]), step=16)            # a piece longer than the step
    assert np.array_equal(one, src[10:4010])


def test_offsets_and_unpack_at_the_sizes_of_the_limits(no_library):
    off = device._offsets(np.full(70_000, 40_000, dtype=np.int64), np.int64, total=True)    # past 2^31: int64 holds
    assert off[-1] == 2_800_000_000 and off.dtype == np.int64
    flags = np.zeros(CAPACITY, dtype=bool)
    flags[[0, 63, 64, LAST]] = True
    words = device._pack(flags)
    assert words.shape == (1024,) and int(words[0]) == 1 | 1 << 63 and int(words[1]) == 1 and int(words[-1]) == 1 << 63
    assert np.array_equal(device._unpack(words, CAPACITY), flags)
    assert device._variant_starts(np.array([2**31], dtype=np.int64), np.array([10])).tolist() == [[12 * 2**31, 12 * 2**31 + 64]]


# ------------------------------------------------------------------ host tier: the coverage conditions, from the models
def test_the_edge_slots_rooms_and_records_are_present_and_distinct(built, edge):
    assert len(set(EDGE_SLOTS)) == 10 and set(EDGE_SLOTS) <= set(edge["slots"]) and len(edge["slots"]) == 10 + limits.RANDOM_SLOTS
    assert EDGE_SLOTS == (0, 255, 256, 257, 32767, 32768, 65279, 65280, 65534, 65535)
    assert edge["rooms"] == list(EDGE_ROOMS) == [0, 1, 511, 1022, 1023] and edge["records"] == list(EDGE_CLONES)
    assert edge["records"] == [0, 63, 64, 255, 256, 32768, 65535]
    users, rooms, records = edge_description()
    assert {records[c][0] for c in EDGE_CLONES} <= set(EDGE_SLOTS)                  # the owners are among the edge slots
    assert edge["hear"] == [0, 1, 2] and edge["ignall_owner"] and 32767 in edge["roomless_away"]
    assert all(r["name"] and r["links"] and r["topic"] and r["netlink"][0] for r in rooms.values())
    named = [u for u in users.values() if u["name"]]
    assert len(named) == len(users) and len({u["name"] for u in named}) == len(named)
    for f, values in (("level", {0, 1, 2, 3, 4}), ("vis", {0, 1}), ("login", {0, 1}), ("afk", {0, 1}), ("ignall", {0, 1}), ("ignshout", {0, 1}),
                      ("igntell", {0, 1}), ("colour", {0, 1})):
        assert {u[f] for u in users.values()} == values, f
    assert any(b"~FBBM" in u["desc"] for u in users.values()) and users[65280]["login"] == 1
    s = edge_script()
    assert set(s["who"]) == {0, LAST, 65280} and {users[j]["room"] for j in s["look"]} == {0, LAST_ROOM}
    assert s["review"] == [LAST_ROOM, 0, LAST_ROOM] and any(b[2] == LAST for b in s["plan"])
    assert {e[0] for e in s["speak"]} <= set(EDGE_SLOTS) and {e[0] for e in s["tell"]} <= set(EDGE_SLOTS)


def test_the_edge_script_reaches_what_it_was_written_for(built, edge):
    assert edge["ring_last_room"] > 0 and edge["revtell_last"] > 0
    assert edge["relays_at_last_record"] >= 1 and edge["clone_sender_last"] == 1
    assert edge["most_colour_coms"] >= 19
    assert edge["tell_outcomes"] == sorted((device.TOLD, device.MUZZLED, device.NOTHING, device.NOBODY, device.SELF, device.AFK,
                                            device.IGNALL, device.IGNTELL, device.OFFSITE))
    assert {0, 256, 257, 32767, 65279, 65534, LAST} == set(edge["tell_targets"])
    assert edge["speech_outcomes"] == [device.SPOKEN, device.MUZZLED, device.NOTHING, device.SWEARING]
    assert edge["read_kinds"] == [device.IAC, device.EMPTY, device.REPEAT, device.UNKNOWN, device.SPEECH, device.COMMAND]


def test_the_full_rosters_counts_are_the_edge(built, full):
    users, rooms = full
    assert len(users) == CAPACITY and all(u["name"] for u in users.values())
    counts = footer_counts(users)
    assert all(10_000 <= n <= 99_999 for n in counts) and counts[0] + counts[1] == counts[2] == len(listed(users))
    assert {u["level"] for u in users.values()} == {0, 1, 2, 3, 4} and {u["room"] for u in users.values()} == {0, 1}
    low, high, prompt = (users[j] for j in FULL_WHO_LOOKERS)
    assert (low["level"], high["level"], prompt["login"]) == (0, 4, 1) and not low["login"] and not high["login"]
    assert len(shown(users, FULL_WHO_LOOKERS[0])) < len(shown(users, FULL_WHO_LOOKERS[1])) == counts[2] > 256 * 250
    assert max(colour_com_count(b"  %s %s~RS" % (u["name"], u["desc"])) for u in users.values()) >= 19
    a, b = (users[j] for j in FULL_LOOKERS)
    assert (a["room"], a["level"], b["room"], b["level"]) == (0, 0, 1, 4)
    assert all(len(members(users, j)) > 10_000 for j in FULL_LOOKERS)


def test_every_tell_case_resolves_to_the_branch_it_is_named_for(built, full):
    users = {j: dict(u) for j, u in full[0].items()}
    first, second = full_tell_cases()
    for name, event, outcome, target in first:
        m = private(users, *event)
        assert (m["outcome"], m["target"]) == (outcome, target), name
    # the exact name lies in the last block and the substring hits before it; the two substring hits in two tiles
    assert users[LAST]["name"] == b"Qzedy" and all(b"Qzedy" in users[j]["name"] != b"Qzedy" for j in (3, 40000))
    assert [j for j, u in users.items() if b"Mark" in u["name"]] == [256, 65280]
    slots, names = full_renames()
    for j, name in zip(slots, names):
        users[j]["name"] = name
    for name, event, outcome, target in second:
        m = private(users, *event)
        assert (m["outcome"], m["target"]) == (outcome, target), name
    assert [j for j, u in users.items() if b"Qzed" in u["name"]] == [LAST]
    assert {c[0] for c in first + second} >= {"exact_in_the_last_block_beats_substrings", "substring_of_the_last_name_alone",
                                              "lowest_substring_wins", "nobody", "exact_target_is_afk", "exact_target_ignores_tells"}


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def limits_run(built):
    res = child_run.run_child("device_limits_child.py", "DEVICE_LIMITS", 900)
    print("\n[limits]", json.dumps(res)[:6000])
    return res


@pytest.mark.gpu
def test_every_call_at_every_limit_at_once_matches_the_models(limits_run):
    e = limits_run["edge"]
    assert e["roster"] == {"capacity": 65536, "look_rooms": 1024, "review_rooms": 1024, "revtell": True, "clones": 65536}
    assert e["n_bad"] == 0, e["first_bad"]
    assert e["comparisons"] > 0 and set(e["by_call"]) == set(CALLS) and all(n > 0 for n in e["by_call"].values()), e["by_call"]
    assert e["slots"] == 10 + limits.RANDOM_SLOTS


@pytest.mark.gpu
def test_the_edge_roster_reached_its_edges_on_the_device(limits_run, edge):
    e = limits_run["edge"]
    assert e["ring_last_room"] == edge["ring_last_room"] > 0
    assert e["revtell_last"] == edge["revtell_last"] > 0 and e["revtell_after_clear"] == 0
    assert e["relays_at_last_record"] >= edge["relays_at_last_record"] >= 1
    assert e["tell_outcomes"] == edge["tell_outcomes"] and set(edge["tell_targets"]) <= set(e["tell_targets"])
    assert e["widest_pad"] >= 40 + 3 * 19                              # some line's colour_com_count is 19 or more


@pytest.mark.gpu
def test_the_full_roster_matches_the_models(limits_run, full):
    f = limits_run["full"]
    assert f["n_bad"] == 0, f["first_bad"]
    assert f["comparisons"] > 0 and all(f["by_call"].get(c, 0) > 0 for c in ("who_many", "look_many", "tell_many", "plan_many",
                                                                           "broadcast_many", "expand")), f["by_call"]
    users = full[0]
    counts = footer_counts(users)
    w = f["who"]
    assert w["lines"] == counts[2] and w["texts"] == 4 + counts[2] and w["bitmap_words"] == 3 * -(-counts[2] // 32)
    assert w["device_footer"] == w["footer"] == ("\nThere are %d visible, %d invisible, 0 remote users.\nTotal of %d users" % tuple(counts))
    assert all(10_000 <= n for n in counts) and w["shown_lines"] > 2 * counts[2]
    assert f["look"]["members"] == f["look"]["model_members"] and min(f["look"]["members"]) > 10_000
    assert sum(f["look"]["lines"]) == CAPACITY
    first, second = full_tell_cases()
    assert f["tell"] == {name: [outcome, -1 if target is None else target] for name, _, outcome, target in first + second}
    assert f["plan"]["bitmap_words"] == 8 * 1024 and max(f["plan"]["admitted"]) > 32_768 and f["plan"]["admitted"][-1] == 0
    b = f["broadcast"]
    assert b["arena_bytes"] == b["model_bytes"] > 1 << 24 and b["arena_items_compared"] >= 2 * (2 + 32)
    assert b["arena_bound"] < device.MANY_ARENA_CAP // 4               # well under the cap


@pytest.mark.gpu
def test_the_accept_side_of_the_size_guards(limits_run):
    g = limits_run["guards"]
    assert g["n_bad"] == 0, g["first_bad"]
    assert g["k"] == GUARD_K and g["cells"] >= 2**28 and g["bitmap_words"] == GUARD_K * 1024 and g["distinct_lines"] == 10
    assert g["comparisons"] >= g["bitmap_words"] + 4 * GUARD_K
    steps = [n for call in g["gather_steps"].values() for n in call]
    assert steps and max(steps) >= 2, g["gather_steps"]                # some _gather crossed its 2^24 step
