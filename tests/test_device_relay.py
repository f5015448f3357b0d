"""``Roster.relay_many``: the clone branch of ``write_room_except`` on the device (nuts_roster_relay of fanout.hip),
``device.Relay``, the clone records (``Roster(clones=)``, ``Roster.set_clones``).

Host tier (unmarked): the new names; everything malformed is rejected before the device library loads, and a rejected call
changes no mirror and no dirty flag; the clone mirror byte for byte; the Python model of the relay (``relays`` and
``relay_text`` of tests/device_relay_child.py) reproduces every relay line of the recorded ``clones`` session; the rules on
hand-built tables; the longest relay text stays within the transducer's bounds on the CPU restatement; a ``Relay`` built by
hand obeys its contract.  The kernel's scratch-free compile is tests/test_device_fanout.py's, which covers every function
of the compiler's report.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_relay_child.py, under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

import child_run
from device_relay_child import (ALL, BROADCASTS_PER_CALL, CAPACITIES, CLONES, NOTHING, SWEARS, longest_text, relay_text, relays,
                                relays_of, replay_relays, swearing)
from nuts333_amd import device, nuts_path

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


def cloned(capacity=4, look_rooms=3, clones=3, **kw) -> device.Roster:
    """A roster with three named rooms, slots 0 .. 2 in rooms 0, 0, 1, and record 0 a clone of slot 2 in room 0."""
    r = device.Roster(capacity, look_rooms=look_rooms, clones=clones, **kw)
    r.update([0, 1, 2], room=[0, 0, 1], name=[b"Alice", b"Bobby", b"Dave"])
    if look_rooms:
        r.set_rooms(list(range(look_rooms)), name=[b"drive", b"hallway", b"N" * 20][:look_rooms])
    if clones and look_rooms:
        r.set_clones(0, owner=2, room=0)
    return r


def state(r):
    """Every mirror's bytes and every dirty flag."""
    names = None if r._relay_names is None else r._relay_names.tobytes()
    return (r._table.tobytes(), r._speech.tobytes(), r._afk.tobytes(), r._rooms.tobytes(), r._udesc.tobytes(), r._clones.tobytes(),
            names, r._dirty, r._speech_dirty, r._private_dirty, r._afk_dirty, r._rooms_dirty, r._udesc_dirty, r._clones_dirty,
            r._clear.tobytes(), r._clear_pending)


BS = [(b"hello\n", 0, 1, 0, 3)]


# ------------------------------------------------------------------ host tier: names and input checks
def test_the_new_names_exist():
    assert device.RELAY_KERNELS == ("nuts_roster_relay",)
    assert (device.CLONE_HEAR_NOTHING, device.CLONE_HEAR_SWEARS, device.CLONE_HEAR_ALL) == (0, 1, 2)
    assert len(device.KERNELS) == 18 and device.KERNELS[-1] == "nuts_roster_look" and "nuts_roster_relay" not in device.KERNELS
    r = device.Roster(2, look_rooms=1, clones=5)
    assert r.clones == 5 and device.Roster(2).clones == 0
    assert callable(r.set_clones) and callable(r.relay_many) and device.Relay.__dataclass_fields__["plan"].type in ("Plan", device.Plan)
    for name in ("relays", "owners", "relay_text", "relay_variant", "relay_chunks"):
        assert callable(getattr(device.Relay, name))


@pytest.mark.parametrize("bad", [-1, device.MAX_CAPACITY + 1, None, "3", 2.0, True])
def test_clones_must_be_a_small_int(no_library, bad):
    with pytest.raises(ValueError, match="clones"):
        device.Roster(4, clones=bad)
    assert device.Roster(4, clones=device.MAX_CAPACITY).clones == device.MAX_CAPACITY


@pytest.mark.parametrize("clones, fields, why", [
    (3, {"owner": 0}, "clone record 3"), (-1, {"owner": 0}, "clone record -1"), (None, {"owner": 0}, "clones must be"),
    ("0", {"owner": 0}, "clones must be"), ([0, True], {"owner": 0}, "clone record True"), ([0, 1.0], {}, "clone record 1.0"),
    (0, {"owner": 4}, "slot"), (0, {"owner": -1}, "slot"), (0, {"owner": "2"}, "owner must be"), (0, {"owner": True}, "slot"),
    ([0, 1], {"owner": [1]}, "1 values for 2 entries"), ([0, 1], {"owner": [1, None, 2]}, "3 values for 2 entries"),
    (0, {"room": 3}, "no room record"), (0, {"room": -1}, "no room record"), (0, {"room": None}, "room must be"),
    ([0, 1], {"owner": [0, 1], "room": [0, 7]}, "room 7 has no room record"),
    (0, {"hear": 3}, "hear must be"), (0, {"hear": -1}, "hear must be"), (0, {"hear": "all"}, "hear must be"),
    (0, {"hear": True}, "hear must be"), ([0, 1, 2], {"owner": 1, "hear": [2, 1, 9]}, "hear must be"),
])
def test_a_rejected_set_clones_changes_nothing(no_library, clones, fields, why):
    r = cloned()
    r._dirty = r._speech_dirty = r._afk_dirty = r._rooms_dirty = r._udesc_dirty = r._clones_dirty = False
    before = state(r)
    with pytest.raises(ValueError, match=why):
        r.set_clones(clones, **fields)
    assert state(r) == before


def test_a_roster_without_clone_records_has_no_relay(no_library):
    r = cloned(clones=0)
    before = state(r)
    with pytest.raises(ValueError, match="no clone records"):
        r.relay_many(BS)
    with pytest.raises(ValueError, match="clone record 0.*clones is 0"):
        r.set_clones(0, owner=1)
    assert state(r) == before


@pytest.mark.parametrize("sender, why", [
    ([None, None], "2 values for 1 broadcasts"), (0, "clone_sender must be"), ("0", "clone_sender must be"), ([3], "clone record 3"),
    ([-1], "clone record -1"), ([True], "clone record True"), ([1.0], "clone record 1.0"), ([0], "its sender must be None"),
])
def test_a_bad_clone_sender_is_rejected(no_library, sender, why):
    r = cloned()
    before = state(r)
    with pytest.raises(ValueError, match=why):
        r.relay_many(BS, clone_sender=sender)
    assert state(r) == before


@pytest.mark.parametrize("ignall, why", [
    ({}, "non-empty dict"), ([1], "non-empty dict"), (1, "non-empty dict"), ({-1: 0}, "ignall: "), ({10**6: 0}, "ignall: "),
    ({1: 2}, "its flag must be 0/1"), ({1: None}, "its flag must be 0/1"), ({1: "1"}, "its flag must be 0/1"),
])
def test_a_bad_ignall_is_rejected(no_library, ignall, why):
    r = cloned()
    before = state(r)
    with pytest.raises(ValueError, match=why):
        r.relay_many(BS, ignall=ignall)
    assert state(r) == before


def test_what_plan_many_rejects_relay_many_rejects(no_library):
    r = cloned()
    before = state(r)
    for bad, why in (([], "empty call"), ("text", "sequence of tuples"), ([(b"x", 0, 9, 0, 3)], "broadcast 0: slot"),
                     ([(b"a\0", 0, None, 0, 3)], "NUL"), ([(b"x", -1, None, 0, 3)], "room"), ([(b"x", 0, None, 2, 3)], "force_listen"),
                     ([(b"x" * 2000, 2, None, 0, 3)], "at most 1999")):
        with pytest.raises(ValueError, match=why):
            r.relay_many(bad)
    with pytest.raises(ValueError, match="no review rings"):
        r.relay_many(BS, record=True)
    with pytest.raises(ValueError, match="closed"):
        with cloned() as c:
            pass
        c.relay_many(BS)
    assert state(r) == before


def test_a_record_needs_a_room_record_and_a_slot(no_library):
    r = cloned()
    r.set_clones(1, owner=1)                             # an owner, and no room yet
    before = state(r)
    with pytest.raises(ValueError, match="clone record 1: its room has no room record"):
        r.relay_many(BS)
    assert state(r) == before
    r.set_clones(1, room=2)
    r._clone_owner[1] = 4                                # past the capacity: set_clones would not have let it in
    before = state(r)
    with pytest.raises(ValueError, match="clone record 1: its owner, slot 4, is out of range"):
        r.relay_many(BS)
    assert state(r) == before
    no_rooms = device.Roster(4, clones=2)
    with pytest.raises(ValueError, match="no room record"):
        no_rooms.set_clones(0, owner=1, room=0)


def test_a_relay_text_must_fit_text2(no_library):
    r = cloned()                                         # record 0 stands in room 0, "drive"; room 2 has the 20-byte name
    assert longest_text(b"drive") == 999 - 12 - 5 == 982 and longest_text(b"N" * 20) == 967
    before = state(r)
    with pytest.raises(ValueError, match=r"broadcast 1: room 0 holds a clone.*1000 bytes.*at most 999"):
        r.relay_many([(b"x" * 982, 0, None, 0, 3), (b"x" * 983, 0, None, 0, 3)])
    assert state(r) == before
    r.set_clones(0, hear=NOTHING)                        # whatever its hear
    with pytest.raises(ValueError, match="holds a clone"):
        r.relay_many([(b"x" * 983, 0, None, 0, 3)])
    r.set_clones(1, owner=0, room=2)
    with pytest.raises(ValueError, match="broadcast 0: room 2 holds a clone"):
        r.relay_many([(b"x" * 968, 2, None, 0, 3)])
    # a room without a clone, and every room at once, take any text: the checks pass and the library is asked for
    for fine in ([(b"x" * 1999, 1, None, 0, 3)], [(b"x" * 1999, None, None, 0, 3)], [(b"x" * 982, 0, None, 0, 3), (b"x" * 967, 2, None, 0, 3)]):
        with pytest.raises(AssertionError, match="library was loaded"):
            r.relay_many(fine)


def test_the_variant_bound_counts_the_relay_texts(no_library, monkeypatch):
    r = cloned()
    bs = [(b"x" * 100, 0, None, 0, 3)]
    assert device._variant_at(100, 1) == 1216 and device._variant_at(100 + 32, 1) == 1600
    monkeypatch.setattr(device, "MANY_ARENA_CAP", 1216 + 1600)
    with pytest.raises(AssertionError, match="library was loaded"):
        r.relay_many(bs)
    monkeypatch.setattr(device, "MANY_ARENA_CAP", 1216 + 1600 - 1)
    before = state(r)
    with pytest.raises(ValueError, match="over the texts and the relay texts is 2816 bytes"):
        r.relay_many(bs)
    monkeypatch.setattr(device, "MANY_ARENA_CAP", 1215)
    with pytest.raises(ValueError, match="variant bound"):
        r.relay_many(bs)
    assert state(r) == before


# ------------------------------------------------------------------ host tier: the mirror
def test_the_clone_mirror_byte_for_byte(no_library):
    r = device.Roster(5, look_rooms=4, clones=3)
    assert r._clones.shape == (27,) and r._clones.dtype == np.uint8
    assert r._clones.tobytes() == b"\xff" * 24 + b"\0" * 3              # owners -1, rooms -1, hear 0
    assert r._clone_owner.base is r._clones and r._clone_room.base is r._clones and r._clone_hear.base is r._clones
    assert r._clones_dirty and r._relay_names is None
    r._dirty = r._speech_dirty = r._afk_dirty = r._rooms_dirty = r._udesc_dirty = r._clones_dirty = False
    others = lambda: (r._dirty, r._speech_dirty, r._private_dirty, r._afk_dirty, r._rooms_dirty, r._udesc_dirty)
    r.set_clones([0, 2, 0], owner=[1, 4, 3], room=[0, 3, 2])            # the last value wins; a new clone hears all
    assert r._clones_dirty and others() == (False,) * 6
    le = lambda *v: b"".join(int(x).to_bytes(4, "little", signed=True) for x in v)
    assert r._clones.tobytes() == le(3, -1, 4) + le(2, -1, 3) + bytes([ALL, 0, ALL])
    r._clones_dirty = False
    r.set_clones(2, hear=SWEARS)
    r.set_clones([0, 1], hear=[NOTHING, SWEARS], room=1)                # a room and a hear for a record without an owner
    assert r._clones.tobytes() == le(3, -1, 4) + le(1, 1, 3) + bytes([NOTHING, SWEARS, SWEARS]) and r._clones_dirty
    r.set_clones(0, owner=3)                                            # given an owner again: a new clone, hears all
    assert r._clone_hear.tolist() == [ALL, SWEARS, SWEARS] and r._clone_room.tolist() == [1, 1, 3]
    r.set_clones(2, owner=0, hear=NOTHING)
    assert r._clone_hear[2] == NOTHING and r._clone_owner[2] == 0
    r.set_clones([2, 1], owner=None, room=2, hear=ALL)                  # emptied, whatever else the entry gives
    assert r._clones.tobytes() == le(3, -1, -1) + le(1, -1, -1) + bytes([ALL, 0, 0])
    r._clones_dirty = False
    r.set_clones([], owner=[])
    r.set_clones(1)
    assert not r._clones_dirty                                          # nothing was set
    r.update(0, room=1, ignall=1, name=b"Zed", desc=b"d", afk_mesg=b"m", afk=1)
    r.set_rooms(0, name=b"drive", topic=b"t")
    assert not r._clones_dirty and r._dirty and r._rooms_dirty          # update and set_rooms do not touch the clone flag
    assert r._table.nbytes == 5 * 5 and r._speech.shape == (5, 16) and r._rooms.nbytes == 4 * 1072     # as they were


# ------------------------------------------------------------------ the model is the reference
def test_the_model_reproduces_every_relay_of_the_clones_session():
    res = replay_relays("clones")
    assert res["mismatches"] == []
    # the figures of the file itself: 34 line steps, 12 recv entries that hold a relay, 14 relay lines in them (two steps
    # relay twice); every one is compared, none is left out
    doc = json.loads((REPO / "tests" / "golden" / "clones.json").read_text())
    entries = sum(any(l.startswith("[ ") and " ]: " in l for l in text.split("\n\r")) for s in doc["steps"]
                  for text in s.get("recv", {}).values())
    assert res["line_steps"] == sum(s["op"] == "line" for s in doc["steps"]) == 34
    assert res["relay_entries"] == res["recorded_entries"] == entries == 12
    assert res["relay_lines"] == res["recorded_lines"] == 14
    assert res["compared_steps"] == [7, 9, 10, 14, 19, 24, 27, 28, 32, 34, 35, 38]
    assert set(res["commands"]) >= {"say", "emote", "go", "clone", "destroy", "switch", "chear", "csay", "ignall", "shout"}


# ------------------------------------------------------------------ the rules, on hand-built tables
def test_each_hear_mode_with_and_without_a_swear_word():
    ignall = {0: 0, 1: 0}
    for hear, clean, dirty in ((NOTHING, [], []), (SWEARS, [], [0]), (ALL, [0], [0])):
        records = [(1, 0, hear)]
        assert relays(records, ignall, 0, None, b"a clean line\n") == clean
        for text in (b"a shit line\n", b"A SHIT LINE\n", b"FuCk", b"xxcUnTxx", b"s" * 900 + b"shit"):
            assert swearing(text) and relays(records, ignall, 0, None, text) == dirty
    assert not swearing(b"sh it fu ck") and not swearing(b"")


def test_the_owners_ignall_and_force_listen():
    records = [(1, 0, ALL), (2, 0, ALL)]
    assert relays(records, {1: 1, 2: 0}, 0, None, b"x") == [1]
    # force_listen cannot override the owner's ignall (c:1417), and com_num plays no part: of a broadcast's tuple the rule
    # reads the text and the room alone
    for force_listen in (0, 1):
        for com in (0, device.COM_SHOUT, device.COM_SEMOTE):
            assert relays_of(records, {1: 1, 2: 0}, (b"x", 0, None, force_listen, com)) == [1]
            assert relays_of(records, {1: 1, 2: 1}, (b"x", 0, 2, force_listen, com)) == []
            assert relays_of(records, {1: 0, 2: 0}, (b"x", 0, 1, force_listen, com)) == [0, 1]     # a slot that sends is no clone


def test_every_room_at_once_the_sender_and_the_order():
    records = [(3, 1, ALL), (1, 0, ALL), (None, 0, ALL), (2, 0, ALL), (1, 1, ALL), (1, 0, ALL)]
    ignall = {1: 0, 2: 0, 3: 0}
    assert relays(records, ignall, None, None, b"a shout") == []                  # rm is None: nothing, never
    assert relays(records, ignall, 0, None, b"x") == [1, 3, 5]                    # two owners' clones, in record order
    assert relays(records, ignall, 0, 3, b"x") == [1, 5] and relays(records, ignall, 0, 0, b"x") == [1, 3, 5]
    assert relays(records, ignall, 1, 4, b"x") == [0] and relays(records, ignall, 2, None, b"x") == []
    # an owner standing in its clone's room gets both lines: the relay does not look at where the owner is
    r = device.Roster(4, look_rooms=2, clones=1)
    r.update(1, room=0)
    assert relays([(1, 0, ALL)], {1: 0}, 0, None, b"both") == [0] and r.table(0, None)[1, device.LISTENER_FIELDS.index("same_room")] == 1


def test_the_relay_text():
    assert relay_text(b"hallway", b"Alice says: hi\n") == b"~FT[ hallway ]:~RS Alice says: hi\n"
    assert nuts_path.transduce(relay_text(b"hallway", b"Alice says: hi\n"), 0) == b"[ hallway ]: Alice says: hi\n\r"
    assert nuts_path.transduce(relay_text(b"d", b"x\n"), 1) == b"\x1b[36m[ d ]:\x1b[0m x\x1b[0m\n\r\x1b[0m"
    for name in (b"d", b"N" * 20):                                                # a name of 1 and of 20 bytes
        longest = b"L" * longest_text(name)
        assert len(relay_text(name, longest)) == device.ARR_SIZE - 1 == 999
        assert len(relay_text(name, b"")) == device.RELAY_EXTRA + len(name) <= device._RELAY_SLACK
    assert device._RELAY_SLACK == device.RELAY_EXTRA + device.ROOM_NAME_LEN == 32
    # a text ending in a slash keeps it: nothing follows it that it could escape
    assert nuts_path.transduce(relay_text(b"d", b"ends in a slash/"), 1) == b"\x1b[36m[ d ]:\x1b[0m ends in a slash/\x1b[0m"


def test_the_longest_relay_text_stays_within_the_bounds():
    most_bytes = most_writes = 0
    for name in (b"d", b"N" * 20, b"\n" * 20, b"~FR" * 6 + b"~F", b"/~" * 10):
        room = longest_text(name)
        for body in (b"\n" * room, (b"~FR" * room)[:room], (b"/~" * room)[:room], b"x" * room, b""):
            text = relay_text(name, body)
            assert len(text) <= device.ARR_SIZE - 1 < device.TEXT_SIZE
            for c in (0, 1):
                ch = nuts_path.chunks(text, c)
                assert sum(map(len, ch)) <= device.max_bytes(len(text)) and len(ch) <= device.MAX_WRITES
                most_bytes, most_writes = max(most_bytes, sum(map(len, ch))), max(most_writes, len(ch))
    assert most_bytes <= device.max_bytes(999) == 5998 and 2 <= most_writes <= device.MAX_WRITES


# ------------------------------------------------------------------ the dataclass
def hand_built_relay():
    """A Relay from the model alone: texts and variants scattered over buffers of 0xAA bytes, -7 in the unused chunk sizes."""
    records = [(1, 0, ALL), (None, 0, ALL), (3, 0, SWEARS), (3, 1, ALL)] + [(None, 0, 0)] * 60 + [(0, 0, ALL)]
    ignall, colour = {0: 0, 1: 0, 3: 0}, {0: 1, 1: 0, 3: 1}
    names = [b"drive", b"hallway"]
    bs = [(b"clean\n", 0, None), (b"a shit one\n", 0, None), (b"every room\n", None, None), (b"~FRred/\n", 1, None), (b"left out\n", 1, 3)]
    k = len(bs)
    bits = np.zeros((k, 2), dtype=np.uint64)
    texts, variants = np.full(400, 0xAA, dtype=np.uint8), np.full(2000, 0xAA, dtype=np.uint8)
    tstarts, tsizes = np.zeros(k, dtype=np.int64), np.full(k, -1, dtype=np.int64)
    starts, sizes = np.zeros((k, 2), dtype=np.int64), np.zeros((k, 2), dtype=np.int64)
    counts, wsz = np.zeros((k, 2), dtype=np.int32), np.full((k, 2, device.MAX_WRITES), -7, dtype=np.int32)
    at, vat, want = 3, 7, []
    for b, (text, rm, cs) in enumerate(bs):
        who = relays(records, ignall, rm, cs, text)
        want.append(who)
        flags = np.zeros(len(records), dtype=bool)
        flags[who] = True
        bits[b] = device._pack(flags)
        if not who:
            continue
        rt = relay_text(names[rm], text)
        tstarts[b], tsizes[b] = at, len(rt)
        texts[at:at + len(rt)] = np.frombuffer(rt, dtype=np.uint8)
        at += len(rt) + 5
        for c in (0, 1):
            ch = nuts_path.chunks(rt, c)
            data = b"".join(ch)
            starts[b, c], sizes[b, c], counts[b, c] = vat, len(data), len(ch)
            variants[vat:vat + len(data)] = np.frombuffer(data, dtype=np.uint8)
            wsz[b, c, :len(ch)] = [len(x) for x in ch]
            vat += len(data) + 3
    owner = np.array([-1 if r[0] is None else r[0] for r in records], dtype=np.int32)
    plan = device.Plan(capacity=4, admitted_bits=np.zeros((k, 1), dtype=np.uint64), colour_bits=np.zeros(1, dtype=np.uint64),
                       variants=np.zeros(0, dtype=np.uint8), variant_starts=np.zeros((k, 2), dtype=np.int64),
                       variant_sizes=np.zeros((k, 2), dtype=np.int64), write_counts=np.zeros((k, 2), dtype=np.int32),
                       write_sizes=np.zeros((k, 2, device.MAX_WRITES), dtype=np.int32))
    rl = device.Relay(plan=plan, clones=len(records), relay_bits=bits, clone_owner=owner,
                      owner_colour=np.array([colour.get(int(o), 0) for o in owner], dtype=np.uint8), texts=texts, text_starts=tstarts,
                      text_sizes=tsizes, variants=variants, variant_starts=starts, variant_sizes=sizes, write_counts=counts,
                      write_sizes=wsz)
    return rl, bs, names, want


def test_a_hand_built_relay_obeys_the_contract(no_library):
    rl, bs, names, want = hand_built_relay()
    assert want == [[0, 64], [0, 2, 64], [], [3], []] and rl.timing == {}
    for b, (text, rm, cs) in enumerate(bs):
        assert rl.relays(b).tolist() == want[b]
        assert rl.owners(b).tolist() == [{0: 1, 2: 3, 3: 3, 64: 0}[c] for c in want[b]]
        rt = relay_text(names[rm], text) if want[b] else b""
        assert rl.relay_text(b) == rt
        for c in (0, 1):
            ch = nuts_path.chunks(rt, c) if want[b] else []
            assert rl.relay_chunks(b, c) == ch and rl.relay_variant(b, c) == b"".join(ch)
    assert rl.owners(1).tolist() == [1, 3, 0] and rl.owner_colours(1).tolist() == [0, 1, 1]
    assert rl.relay_text(2) == b"" and rl.relay_chunks(2, 1) == [] and rl.owners(4).tolist() == []
    assert rl.relay_variant(3, 1).startswith(b"\x1b[36m[ hallway ]:\x1b[0m \x1b[31mred")
    for bad_k in (-1, 5):
        for call in (rl.relays, rl.owners, rl.owner_colours, rl.relay_text, lambda k: rl.relay_variant(k, 0), lambda k: rl.relay_chunks(k, 1)):
            with pytest.raises(IndexError):
                call(bad_k)
    for call in (rl.relay_variant, rl.relay_chunks):
        with pytest.raises(IndexError):
            call(0, 2)


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def relay_run(built):
    res = child_run.run_child("device_relay_child.py", "DEVICE_RELAY", 300)
    print("\n[relay]", json.dumps(res)[:4000])
    return res


@pytest.mark.gpu
def test_seeded_relays_match_the_model(relay_run):
    f = relay_run["fuzz"]
    assert f["capacities"] == list(CAPACITIES) == [1, 64, 65, 257] and f["clones"] == list(CLONES) == [1, 63, 64, 65, 257]
    assert f["calls"] == 2 * len(CAPACITIES) * len(CLONES) and f["broadcasts"] == f["calls"] * BROADCASTS_PER_CALL
    assert BROADCASTS_PER_CALL == 32
    assert f["hear"] == [NOTHING, SWEARS, ALL] and f["owner_colours"] == [0, 1]
    for what in ("rm_none", "no_clone_room", "empty_text", "clone_sender", "clone_sender_excluded", "ignall_owner",
                 "forced_past_ignall", "swear_relays", "relays", "at_limit"):
        assert f[what] > 0, what
    # relays in several bitmap words of one broadcast, and at the records on either side of a word's and a tile's edge
    assert f["most_relays"] > 16 and f["most_words"] >= 4 and f["edge_relays"] > 0
    assert f["n_bad"] == 0, f["first_bad"]


@pytest.mark.gpu
def test_the_plan_is_plan_manys_and_the_variants_are_the_relay_texts(relay_run):
    c = relay_run["contract"]
    assert c["with_relays"] > 0 and c["without"] > 0 and c["recorded_lines"] > 0
    assert c["n_bad"] == 0, c["first_bad"]


@pytest.mark.gpu
def test_a_second_run_gives_identical_bytes(relay_run):
    assert relay_run["determinism"] == {"same_on_a_second_call": True, "same_on_a_second_roster": True}


@pytest.mark.gpu
def test_nothing_else_moved(relay_run):
    m = relay_run["moved"]
    assert m["with_clones"] == m["fresh"]                               # results and copy volumes alike
    assert m["timing_keys"][0] == m["timing_keys"][1] == m["timing_keys"][2] == ["d2h_bytes", "end_to_end_us", "h2d_bytes", "kernels_us"]
    assert m["relays"] == [35, 0, 35]                                   # 70 records over two rooms; every room at once: none
    # ... and after relay_many calls the other calls still return what they return on the fresh roster; a call may copy
    # less there, never more: a relay call that found the allocation grown has uploaded the table again already
    for call, parts in m["fresh_again"].items():
        assert m["after_relaying"][call][:-1] == parts[:-1], call
        assert all(x <= y for x, y in zip(m["after_relaying"][call][-1], parts[-1])), call
    h, cap, clones, rooms, k = m["relay_h2d"], m["capacity"], m["clones"], m["look_rooms"], m["broadcasts"]
    slice_of = lambda n: -(-n // 256) * 256                             # an array's 256-byte aligned slice of the upload
    # clean tables: the texts, eight small arrays per broadcast (offsets, lengths, rooms, senders, flags, commands, clone
    # senders, the relay texts' offsets) and the violation count; what plan_many uploads, and two arrays more
    clean = slice_of(m["text_bytes"]) + slice_of(4 * k) * 7 + slice_of(k) + 4
    assert h["clean"] == [clean, clean] and h["clean_again"] == clean == h["after_set_rooms_of_no_name"]
    assert h["plan_clean"] == clean - 2 * slice_of(4 * k)
    # after set_clones alone: the records' 9 bytes each, in three slices, and nothing else
    assert h["after_set_clones"] - clean == 2 * slice_of(4 * clones) + slice_of(clones)
    assert 9 * clones <= h["after_set_clones"] - clean < 9 * clones + 3 * 256
    # a new room name: the names, 24 bytes per look room, lie in front of the records, which travel with them
    assert h["after_a_new_name"] - h["after_set_clones"] == slice_of(24 * rooms)
    # an update of the table: its 5 bytes per slot in two slices, and neither the names nor the records behind it
    assert h["after_update"] - clean == slice_of(4 * cap) + slice_of(cap)
    assert h["first"] >= h["after_a_new_name"]
