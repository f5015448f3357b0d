"""A resident listener roster: ``device.Roster`` and nuts_roster_{measure,emit} of fanout.hip.

Host tier (unmarked): malformed rosters, updates and calls are rejected before the device library loads; ``table()``
gives the listener table a broadcast() of the same broadcast would take, and through the restatement's predicate it
admits what write_room_except admits (nuts333.c:1401-1415); a slot given twice in one update takes its last values.
The kernels' scratch-free compile is tests/test_device_fanout.py's, over every name in ``device.KERNELS``.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_roster_child.py, under ``timeout``), and the tests assert on its JSON: random calls and updates against
the CPU restatement and against ``broadcast_many`` over ``table()``, updates taking effect, no table upload when nothing
changed, isolation between rosters, the bench step and the worst case.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import child_run
from nuts333_amd import device, nuts_path

COL = device.LISTENER_FIELDS.index


# ------------------------------------------------------------------ host tier
@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


def roster(capacity=8):
    r = device.Roster(capacity)
    r.update(range(capacity), room=0)
    return r


@pytest.mark.parametrize("capacity", [0, 65537, -1, 2.0, True, "8", None])
def test_roster_rejects_a_bad_capacity(no_library, capacity):
    with pytest.raises(ValueError):
        device.Roster(capacity)


def test_roster_capacity_bounds_are_accepted(no_library):
    assert device.Roster(1).capacity == 1 and device.Roster(device.MAX_CAPACITY).capacity == 65536
    assert device.Roster(1).table(None, None).tolist() == [[0] * 7]      # a new slot is empty


@pytest.mark.parametrize("slots, fields", [
    ([8], {"room": 0}),                          # slot out of range
    ([-1], {"room": 0}),
    ([0, 8], {"colour": 1}),
    ([True], {"room": 0}),                       # not a slot
    ([0.0], {"room": 0}),
    ("ab", {"room": 0}),
    ([0], {"room": -1}),                         # a room outside [0, 2**31 - 1)
    ([0], {"room": 2**31}),
    ([0], {"room": 2**31 - 1}),
    ([0], {"room": True}),
    ([0], {"room": "1"}),
    ([0, 1], {"room": [0, -1]}),
    ([0], {"login": 2}),                         # a flag that is not 0/1
    ([0], {"ignall": -1}),
    ([0], {"colour": 0.5}),
    ([0, 1], {"ignshout": [0, 2]}),
    ([0, 1], {"room": [0, 1, 2]}),               # mismatched lengths
    ([0, 1, 2], {"colour": [1, 0]}),
    ([0], {"colour": [1, 0]}),
    ([0, 1], {"room": 0, "login": [1]}),
    ([0], {"colour": "1"}),
])
def test_update_rejects_malformed_input_and_changes_nothing(no_library, slots, fields):
    r = roster()
    before = r._table.copy()
    with pytest.raises(ValueError):
        r.update(slots, **fields)
    assert np.array_equal(r._table, before)


def test_update_rejects_an_unknown_field(no_library):
    with pytest.raises(TypeError):
        roster().update([0], present=1)


GOOD = (b"hi\n", 0, None, 0, device.COM_SAY)


@pytest.mark.parametrize("call", [
    [],                                          # no broadcasts
    (),
    b"hi\n",                                     # not a sequence of tuples
    42,
    [(b"hi\n", 0, None, 0)],                     # four fields
    [GOOD + (0,)],                               # six
    [list(GOOD)],                                # not a tuple
    [GOOD, (b"hi\n", 0)],
])
def test_broadcast_many_rejects_malformed_calls_before_the_device(no_library, call):
    with pytest.raises(ValueError):
        roster().broadcast_many(call)


@pytest.mark.parametrize("bad", [
    (b"hi\n", 0, 8, 0, 3),                                       # sender equal to capacity
    (b"hi\n", 0, -1, 0, 3),                                      # sender: None, not -1
    (b"hi\n", 0, True, 0, 3),
    (b"hi\n", -1, None, 0, 3),                                   # rm: None, not -1
    (b"hi\n", 2**31, None, 0, 3),
    (b"hi\n", "0", None, 0, 3),
    (b"hi\n", 0, None, 2, 3),                                    # force_listen not a flag
    (b"hi\n", 0, None, 0, 92),                                   # no such command
    (b"hi\n", 0, None, 0, True),
    (b"h\0i\n", 0, None, 0, 3),                                  # NUL
    (b"y" * 2000, 0, None, 0, 4),                                # too long
    ("caf€", 0, None, 0, 3),                                     # not one byte per character
    (42, 0, None, 0, 3),                                         # not text
])
def test_broadcast_many_rejects_one_bad_broadcast_among_good_ones(no_library, bad):
    with pytest.raises(ValueError, match=r"^broadcast 1: "):
        roster().broadcast_many([GOOD, bad, GOOD])


def test_broadcast_many_rejects_a_call_over_the_cap(no_library):
    text = b"\n" * 1999
    per = device.max_bytes(len(text))
    r = device.Roster(device.MAX_CAPACITY)
    r.update(range(device.MAX_CAPACITY), room=0)
    k = device.MANY_ARENA_CAP // (device.MAX_CAPACITY * per)        # the most broadcasts at the cap
    with pytest.raises(ValueError, match="MANY_ARENA_CAP"):
        r.broadcast_many([(text, 0, None, 0, device.COM_SAY)] * (k + 1))
    r._prepare([(text, 0, None, 0, device.COM_SAY)] * k)            # at the cap the call is packed, not refused
    # the bound counts only slots with a room: with most slots out of every room the same call is packed
    r.update(range(1000, device.MAX_CAPACITY), room=None)
    r._prepare([(text, 0, None, 0, device.COM_SAY)] * (k + 1))
    big = device.Roster(1 << 16)
    with pytest.raises(ValueError, match="2\\^31"):                 # K x capacity
        big._prepare([GOOD] * (1 << 15))


def test_a_closed_roster_raises(no_library):
    with roster() as r:
        pass
    for use in (lambda: r.update([0], room=1), lambda: r.table(0, None), lambda: r.broadcast_many([GOOD])):
        with pytest.raises(ValueError, match="closed"):
            use()
    r.close()                                                          # closing twice is harmless


def test_prepare_packs_texts_rooms_senders_flags_and_commands(no_library):
    r = roster()
    text, text_off, lens, rm, sender, flags, coms = r._prepare([
        (b"ab\n", 3, 7, 1, device.COM_SHOUT), ("", None, None, 0, device.COM_SAY),
        (b"xyz", 0, 0, True, device.COM_SEMOTE)])
    assert text == b"ab\nxyz" and text_off.tolist() == [0, 3, 3] and lens.tolist() == [3, 0, 3]
    assert rm.tolist() == [3, -1, 0] and sender.tolist() == [7, -1, 0] and flags.tolist() == [2, 0, 2]
    assert coms.tolist() == [device.COM_SHOUT, device.COM_SAY, device.COM_SEMOTE]


def hand_built():
    """Six slots: 0 room 1 colour; 1 room 1 ignshout; 2 room 2 ignall; 3 room 1 logging in; 4 no room; 5 room 2
    colour and ignshout."""
    r = device.Roster(6)
    r.update([0, 1, 2, 3, 5], room=[1, 1, 2, 1, 2])
    r.update([0, 5], colour=1)
    r.update([1, 5], ignshout=True)
    r.update(2, ignall=1)
    r.update(3, login=1)
    return r


#              login has_room same_room ignall ignshout is_sender colour
ROWS = {0: [0, 1, 0, 0, 0, 0, 1], 1: [0, 1, 0, 0, 1, 0, 0], 2: [0, 1, 0, 1, 0, 0, 0], 3: [1, 1, 0, 0, 0, 0, 0],
        4: [0, 0, 0, 0, 0, 0, 0], 5: [0, 1, 0, 0, 1, 0, 1]}


@pytest.mark.parametrize("rm, sender", [(1, 0), (1, None), (None, 5), (None, None), (2, 4), (7, None)])
def test_table_gives_exactly_the_expected_rows(no_library, rm, sender):
    rooms = {0: 1, 1: 1, 2: 2, 3: 1, 4: None, 5: 2}
    want = np.array([ROWS[j] for j in range(6)], dtype=np.uint8)
    for j in range(6):
        want[j, COL("same_room")] = rm is not None and rooms[j] == rm
        want[j, COL("is_sender")] = j == sender
    t = hand_built().table(rm, sender)
    assert t.dtype == np.uint8 and t.shape == (6, 7)
    assert t.tolist() == want.tolist()


@pytest.mark.parametrize("com", [device.COM_SAY, device.COM_SHOUT])
@pytest.mark.parametrize("force_listen", [0, 1])
def test_table_admits_what_write_room_except_admits(no_library, com, force_listen):
    r = hand_built()

    def admitted(rm, sender):
        return [j for j, row in enumerate(r.table(rm, sender).tolist())
                if nuts_path.admits(row[:6], rm is None, force_listen, com)]
    shout = com == device.COM_SHOUT
    # room 1 from slot 0: slot 1 unless ignshout applies, never the logging-in slot 3 or the sender
    assert admitted(1, 0) == ([] if shout else [1])
    # every room, no sender: every slot with a room that is not logging in, filtered by ignall / ignshout
    want = [j for j in (0, 1, 2, 5) if not (shout and j in (1, 5)) and not (j == 2 and not force_listen)]
    assert admitted(None, None) == want
    # slot 4 has no room: never admitted, whatever the room or the sender
    assert all(4 not in admitted(rm, s) for rm in (None, 0, 1, 2) for s in (None, 0, 4))
    assert admitted(9, None) == []                                     # a room nobody is in


def test_repeated_slots_resolve_as_last_write_wins(no_library):
    r = device.Roster(4)
    r.update([1, 2, 1, 1], room=[5, 6, 7, 8], colour=[1, 1, 0, 1], login=[0, 1, 1, 0])
    assert r.table(None, None)[:, [COL("has_room"), COL("login"), COL("colour")]].tolist() == [
        [0, 0, 0], [1, 0, 1], [1, 1, 1], [0, 0, 0]]
    assert r.table(8, None)[:, COL("same_room")].tolist() == [0, 1, 0, 0]
    r.update([3, 3], room=[4, None])
    r.update(1, colour=0)                                              # a field not given stays as it is
    t = r.table(8, None)
    assert t[3].tolist() == [0] * 7 and t[1].tolist() == [0, 1, 1, 0, 0, 0, 0]


def test_building_and_updating_does_not_touch_the_device(no_library):
    r = device.Roster(1000)
    r.update(range(0, 1000, 2), room=3, colour=1, ignall=0)
    r.table(3, 0)
    r._prepare([GOOD])
    r.close()


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def roster_run(built):
    res = child_run.run_child("device_roster_child.py", "DEVICE_ROSTER", 900)
    print("\n[roster]", json.dumps(res)[:1500])
    return res


@pytest.mark.gpu
def test_random_calls_and_updates_match_the_restatement_and_broadcast_many(roster_run):
    r = roster_run["random"]
    assert sorted(set(r["capacities"])) == [1, 2, 255, 256, 257, 1000, 1015, 4096]
    assert set(r["ks"]) >= {1, 7, 100, 1000} and r["calls"] >= 32 and r["items"] >= 1_000_000
    assert r["calls_without_update"] > 0 and r["updates"] > 0
    # every record a slot can have (same_room needs has_room: 96 of 128), both rm forms, both sender forms
    assert r["records_seen"] == 96 and r["rm_forms"] == ["every room", "room"]
    assert r["sender_forms"] == ["none", "slot"]
    assert r["n_bad_cpu"] == 0, r["first_bad_cpu"]
    assert r["n_bad_tables"] == 0, r["first_bad_tables"]


@pytest.mark.gpu
def test_updates_take_effect_on_exactly_their_slot(roster_run):
    u = roster_run["updates"]
    assert [c["field"] for c in u] == ["colour", "room", "ignshout"]
    for c in u:
        assert c["changed_slots"] == [c["slot"]], c
        assert c["earlier_result_unchanged"] is True, c
        assert c["n_bad"] == 0, c


@pytest.mark.gpu
def test_no_change_calls_upload_no_table(roster_run):
    h = roster_run["h2d"]
    assert h["clean"]["256"] == h["clean"]["4096"] > 0
    for cap in ("256", "4096"):
        assert h["dirty"][cap] - h["clean"][cap] == 5 * int(cap), h
        assert h["after_update"][cap] == h["dirty"][cap] and h["clean_again"][cap] == h["clean"][cap], h


@pytest.mark.gpu
def test_rosters_are_isolated_from_each_other_and_from_other_calls(roster_run):
    i = roster_run["isolation"]
    assert i["a_repeat_identical"] is True and i["b_repeat_identical"] is True
    assert i["n_bad"] == 0 and i["a_differs_from_b"] is True


@pytest.mark.gpu
def test_bench_step_of_100_shouts_to_a_1000_slot_roster(roster_run):
    b = roster_run["bench_step"]
    assert b["broadcasts"] == 100 and b["deliveries"] == 99_900
    assert b["n_bad"] == 0, b["first_bad"]
    t = b["timing"]
    assert 0 < t["kernels_us"] <= t["end_to_end_us"] and t["h2d_bytes"] > 0 and t["d2h_bytes"] > b["bytes"]


@pytest.mark.gpu
def test_worst_case_items_and_buffer_reuse(roster_run):
    w = roster_run["worst"]
    assert w["items"] == 64 * 64 and w["per_item"] == [[11_998, 14]]
    assert w["n_bad"] == 0, w["first_bad"]
    assert w["reuse_identical"] is True
