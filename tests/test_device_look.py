"""``Roster.look_many``: look() composed over the roster on the device (nuts_roster_look of fanout.hip), ``device.Look``,
the room table (``Roster(look_rooms=)``, ``Roster.set_rooms``) and the users' ``desc`` (``Roster.update(desc=)``).

Host tier (unmarked): everything malformed is rejected before the device library loads, and a rejected call changes no
mirror and no dirty flag; the room record, the description row and the slot row byte for byte; the Python model of
``look()`` (``look`` of tests/device_look_child.py) reproduces every look of twelve recorded sessions; the rules of the
member list and of the room texts on hand-built rosters; a member line, and the five room texts at their worst, stay
within their bounds on the CPU restatement; a ``Look`` built by hand obeys its contract.  The kernels' scratch-free
compile is tests/test_device_fanout.py's, over every name in ``device.KERNELS``.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_look_child.py, under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import itertools
import json

import numpy as np
import pytest

import child_run
from device_look_child import (CAPACITIES, GOLDEN, LOOKERS_PER_CALL, WORST_DESCS, WORST_NAMES, fuzz_rooms, golden_looks, look,
                               look_user, member_line, members, model_answer, model_chunks, new_room, replay_looks)
from nuts333_amd import device, nuts_path


def roomed(capacity=4, look_rooms=3, **kw) -> device.Roster:
    """A roster with three room records whose slots 0 and 1 stand in room 0."""
    r = device.Roster(capacity, look_rooms=look_rooms, **kw)
    r.update([0, 1], room=0, name=[b"Alice", "Bobby"])
    return r


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


def flags(r):
    return (r._dirty, r._speech_dirty, r._private_dirty, r._afk_dirty, r._rooms_dirty, r._udesc_dirty)


# ------------------------------------------------------------------ host tier: input checks
def test_the_new_names_exist():
    assert device.KERNELS[-1] == "nuts_roster_look" and len(device.KERNELS) == 18
    assert device.MAX_LOOK_ROOMS == device.MAX_REVIEW_ROOMS == 1024
    assert (device.ROOM_NAME_LEN, device.ROOM_DESC_LEN, device.MAX_LINKS, device.TOPIC_LEN, device.SERV_NAME_LEN,
            device.USER_DESC_LEN) == (20, 810, 10, 60, 80, 30)
    assert (device.PUBLIC, device.PRIVATE, device.FIXED_PUBLIC, device.FIXED_PRIVATE) == (0, 1, 2, 3)
    assert (device.MAX_MEMBER_BYTES, device.MAX_MEMBER_WRITES) == (294, 2)


@pytest.mark.parametrize("bad", [-1, 1025, None, "3", 2.0, True])
def test_look_rooms_must_be_a_small_int(no_library, bad):
    with pytest.raises(ValueError, match="look_rooms"):
        device.Roster(4, look_rooms=bad)
    assert device.Roster(4, look_rooms=1024).look_rooms == 1024 and device.Roster(4).look_rooms == 0


@pytest.mark.parametrize("rooms, fields, why", [
    (3, {"name": b"x"}, "no room record"), (-1, {"name": b"x"}, "no room record"), (None, {"name": b"x"}, "rooms must be"),
    ("0", {"name": b"x"}, "rooms must be"), ([0, True], {"name": b"x"}, "no room record"), ([0, 1.0], {}, "no room record"),
    (0, {"name": b"n" * 21}, "^room 0: name"), ([0, 1], {"name": [b"ok", b"a\0b"]}, "^room 1: name"), (0, {"name": 5}, "name must be"),
    (0, {"name": "Ā"}, "outside one byte"), ([0, 1], {"name": [b"one"]}, "1 values for 2 rooms"),
    (0, {"access": 4}, "^room 0: access"), (0, {"access": -1}, "access"), (0, {"access": "PUB"}, "access"),
    ([0, 1], {"access": [0, True]}, "^room 1: access"), (0, {"access": None}, "access"),
    (0, {"desc": b"d" * 811}, "^room 0: desc"), (0, {"desc": b"a\0"}, "desc"), ([0, 1, 2], {"desc": [b"", b"", 7]}, "^room 2: desc"),
    (0, {"links": [3]}, "^room 0: room 3 has no room record"), (0, {"links": [0] * 11}, "at most 10"), (0, {"links": 1}, "links"),
    ([0, 1], {"links": [[1], [0, -1]]}, "^room 1: room -1"), (0, {"links": "12"}, "links"), ([0, 1], {"links": [[1]]}, "1 values for 2 rooms"),
    (0, {"topic": b"t" * 61}, "^room 0: topic"), (0, {"topic": None}, "topic"),
    (0, {"mesg_cnt": -1}, "mesg_cnt"), (0, {"mesg_cnt": 2**31}, "mesg_cnt"), (0, {"mesg_cnt": 1.5}, "mesg_cnt"),
    (0, {"mesg_cnt": True}, "mesg_cnt"),
    (0, {"netlink": ("svc", 1)}, "netlink"), (0, {"netlink": (b"s" * 81, True)}, "netlink service"), (0, {"netlink": "svc"}, "netlink"),
    ([0, 1], {"netlink": [None, (b"a\0", False)]}, "^room 1: netlink service"), (0, {"netlink": (b"svc",)}, "netlink"),
    ([0, 1], {"name": b"fine", "topic": [b"ok", b"t" * 61]}, "^room 1: topic"),
])
def test_a_rejected_set_rooms_changes_nothing(no_library, rooms, fields, why):
    r = roomed()
    r.set_rooms([0, 1, 2], name=[b"drive", b"hall", b"wiz"], links=[[1], [0, 2], [1]], desc=b"A room.\n")
    r._dirty = r._speech_dirty = r._afk_dirty = r._rooms_dirty = r._udesc_dirty = False
    before = r._rooms.copy()
    with pytest.raises(ValueError, match=why):
        r.set_rooms(rooms, **fields)
    assert np.array_equal(r._rooms, before) and flags(r) == (False,) * 6


@pytest.mark.parametrize("fields", [{"desc": b"d" * 31}, {"desc": b"a\0b"}, {"desc": 5}, {"desc": None}, {"desc": "Ā"},
                                    {"desc": [b"ok"]}, {"desc": [b"ok", b"d" * 31]}, {"desc": b"fine", "level": 9},
                                    {"desc": b"fine", "room": -2}])
def test_a_rejected_update_of_desc_changes_no_mirror(no_library, fields):
    r = roomed()
    r.update([0, 1], desc=[b"is alice", b"is bobby"])
    r._dirty = r._speech_dirty = r._afk_dirty = r._rooms_dirty = r._udesc_dirty = False
    table, speech, udesc = r._table.copy(), r._speech.copy(), r._udesc.copy()
    with pytest.raises(ValueError):
        r.update([0, 1], **fields)
    assert np.array_equal(r._table, table) and np.array_equal(r._speech, speech) and np.array_equal(r._udesc, udesc)
    assert flags(r) == (False,) * 6


@pytest.mark.parametrize("slots", [[], (), None, 3, "01", b"01"])
def test_slots_must_be_a_non_empty_sequence(no_library, slots):
    with pytest.raises(ValueError, match="slots|empty call"):
        roomed().look_many(slots)


def test_a_looker_needs_a_room_with_a_record(no_library):
    r = roomed()
    r.update(2, room=3, name=b"Carol")                   # room 3 has no record
    for bad, why in (([0, 4], "look 1: slot"), ([0, 1, -1], "look 2: slot"), ([None], "look 0: slot"), ([True], "look 0: slot"),
                     ([1, 0, 3], "look 2: .*slot 3, is in no room"), ([2], "look 0: .*room 3, which has no room record")):
        with pytest.raises(ValueError, match=why):
            r.look_many(bad)
    with pytest.raises(ValueError, match=r"look 0: .*look_rooms is 0"):
        device.Roster(2).look_many([0])
    assert flags(r)[4:] == (True, True)                  # nothing was uploaded


def test_a_closed_roster_raises(no_library):
    with roomed() as r:
        pass
    for call in (lambda: r.look_many([0]), lambda: r.set_rooms(0, name=b"x"), lambda: r.update(0, desc=b"x")):
        with pytest.raises(ValueError, match="closed"):
            call()


# ------------------------------------------------------------------ host tier: the layouts
def test_the_room_record_the_desc_row_and_the_slot_row_byte_for_byte(no_library):
    r = device.Roster(3, look_rooms=4)
    assert r._rooms.shape == (4 * (256 + 816),) and r._rooms.dtype == np.uint8 and not r._rooms.any()
    assert r._room_rec.shape == (4, 256) and r._room_desc.shape == (4, 816) and r._udesc.shape == (3, 32) and not r._udesc.any()
    assert r._room_rec.base is r._rooms and r._room_desc.base is r._rooms      # one upload: the records, then the rows
    assert flags(r) == (True, True, False, True, True, True)
    r._dirty = r._speech_dirty = r._afk_dirty = r._rooms_dirty = r._udesc_dirty = False
    r.set_rooms([1, 3, 1], name=[b"first", b"N" * 20, b"hall"], access=[0, 3, 1], links=[[0], [2, 1, 0], [3, 3]],
                topic=[b"", b"T" * 60, b"chat"], mesg_cnt=[0, 2**31 - 1, 258], netlink=[None, (b"S" * 80, True), (b"peer", False)],
                desc=[b"", b"D" * 810, b"two\nlines\n"])
    assert flags(r) == (False, False, False, False, True, False)               # the room table alone
    rec = r._room_rec[1].tobytes()                                             # the last values win
    assert rec[:20] == b"hall" + b"\0" * 16 and rec[20:28] == bytes([4, 1, 2, 4, 1, 4, 10, 0])
    assert rec[28:32] == (258).to_bytes(4, "little") and rec[32:40] == (3).to_bytes(4, "little") * 2 and not any(rec[40:72])
    assert rec[72:132] == b"chat" + b"\0" * 56 and rec[132:212] == b"peer" + b"\0" * 76 and not any(rec[212:])
    assert r._room_desc[1].tobytes() == b"two\nlines\n" + b"\0" * 806
    rec = r._room_rec[3].tobytes()
    assert rec[:28] == b"N" * 20 + bytes([20, 3, 3, 60, 3, 80]) + (810).to_bytes(2, "little")
    assert rec[28:32] == (2**31 - 1).to_bytes(4, "little") and rec[32:44] == b"".join(x.to_bytes(4, "little") for x in (2, 1, 0))
    assert rec[72:132] == b"T" * 60 and rec[132:212] == b"S" * 80 and not any(rec[212:])
    assert r._room_desc[3].tobytes() == b"D" * 810 + b"\0" * 6 and not r._room_rec[[0, 2]].any() and not r._room_desc[[0, 2]].any()
    r.set_rooms(3, netlink=None, topic=b"", links=[], desc=b"")                # and everything can be taken back
    rec = r._room_rec[3].tobytes()
    assert rec[20:28] == bytes([20, 3, 0, 0, 0, 0, 0, 0]) and not any(rec[32:212]) and not r._room_desc[3].any()
    r._rooms_dirty = False
    r.set_rooms([], name=[])
    r.set_rooms(0)
    assert flags(r) == (False,) * 6                                            # nothing was set
    r.update([2, 0, 2], desc=[b"first", "d" * 30, b"is ~FRred/"])
    assert flags(r) == (False, False, False, False, False, True)               # the descriptions alone
    assert r._udesc[2].tobytes() == b"is ~FRred/" + b"\0" * 20 + bytes([10, 0])
    assert r._udesc[0].tobytes() == b"d" * 30 + bytes([30, 0]) and not r._udesc[1].any()
    r.update(0, desc=b"")
    assert not r._udesc[0].any()
    assert r._speech.shape == (3, 16) and r._afk.shape == (3, 64) and r._table.nbytes == 5 * 3     # as they were


# ------------------------------------------------------------------ the model is the reference
@pytest.mark.parametrize("name", GOLDEN)
def test_the_model_reproduces_every_recorded_look(name):
    res = replay_looks(name, model_answer)
    assert res["mismatches"] == []
    assert res["compared"] == golden_looks(name) > 0                    # it leaves out no look of the session


def test_the_replay_covers_rooms_and_enough_more():
    named = {"prompts", "errors", "filters", "afk_bcast", "speech_colour_off", "speech_colour_mixed", "login_paths", "capacity",
             "charecho", "markup", "review", "swearing", "framing", "long_motd"}
    assert "rooms" in GOLDEN and len(named & set(GOLDEN)) >= 7 and len(set(GOLDEN)) == len(GOLDEN)
    total = sum(golden_looks(name) for name in GOLDEN)
    assert total == 49 >= 40
    assert sum(golden_looks(n) for n in ("rooms", "prompts", "errors", "filters", "afk_bcast", "speech_colour_off",
                                         "speech_colour_mixed", "login_paths")) == 43      # the figure of the issue
    kinds = {}
    for name in GOLDEN:
        for kind, n in replay_looks(name, model_answer)["kinds"].items():
            kinds[kind] = kinds.get(kind, 0) + n
    assert kinds == {"login": 35, "go": 8, "look": 6}


# ------------------------------------------------------------------ the rules, on hand-built rosters
def people(rooms=None):
    users = {j: look_user(j, name=b"U%d" % j) for j in range(4)}
    return users, rooms or [new_room(b"here")]


def test_who_is_listed_for_every_pair_of_levels():
    for lu, lj, vis in itertools.product(range(5), range(5), (0, 1)):
        users, rooms = people()
        users[0]["level"], users[1]["level"], users[1]["vis"] = lu, lj, vis
        users[2]["room"] = users[3]["room"] = None
        seen = bool(vis or lj <= lu)
        assert members(users, 0) == ([1] if seen else [])
        texts = look(users, rooms, 0)
        if seen:
            assert texts[3] == b"~FTYou can see:\n" and len(texts) == 8
            assert texts[4] == (b"      U1 ~RS  \n" if vis else b"     ~FR*~RSU1 ~RS  \n") == member_line(users[1])
        else:
            assert texts[3] == b"~FTYou are all alone here.\n" and len(texts) == 7


def test_the_order_the_afk_mark_and_who_is_no_member():
    users, rooms = people()
    users[3].update(afk=1, desc=b"is three")
    users[2].update(name=None)                                          # a slot without a name is not a user
    users[1].update(room=None)
    assert members(users, 0) == [3] and members(users, 3) == [0]        # never oneself
    assert look(users, rooms, 0)[4] == b"      U3 is three~RS  ~BR(AFK)\n"
    users[1].update(room=0, vis=0, level=1)
    users[2].update(name=b"Two", login=1)                               # login is not consulted
    assert members(users, 0) == [1, 2, 3] and members(users, 2) == [0, 1, 3]
    assert look(users, rooms, 0)[3:7] == [b"~FTYou can see:\n", b"     ~FR*~RSU1 ~RS  \n", b"      Two ~RS  \n",
                                           b"      U3 is three~RS  ~BR(AFK)\n"]
    assert look(users, rooms, 0)[7] == b"\n"


def test_a_slash_before_the_lines_rs_makes_it_literal():
    users, rooms = people()
    users[1]["desc"] = b"ends in a slash/"
    line = look(users, rooms, 0)[4]
    assert line == b"      U1 ends in a slash/~RS  \n"
    assert nuts_path.transduce(line, 1) == b"      U1 ends in a slash~RS  \x1b[0m\n\r\x1b[0m"     # transduced whole
    assert nuts_path.transduce(line, 0) == b"      U1 ends in a slash~RS  \n\r"
    users[1]["desc"] = b"plain"
    assert nuts_path.transduce(look(users, rooms, 0)[4], 0) == b"      U1 plain  \n\r"


def test_the_room_texts():
    rooms = [new_room(b"pub"), new_room(b"priv", access=device.PRIVATE), new_room(b"fpub", access=device.FIXED_PUBLIC),
             new_room(b"fpriv", access=device.FIXED_PRIVATE)]
    users = {0: look_user(0, name=b"A")}
    want = {0: (b"~FG", b"set to ~FGPUBLIC~RS"), 1: (b"~FR", b"set to ~FRPRIVATE~RS"), 2: (b"~FG", b"~FRfixed~RS to ~FGPUBLIC~RS"),
            3: (b"~FR", b"~FRfixed~RS to ~FRPRIVATE~RS")}
    for rm, (mark, words) in want.items():
        users[0]["room"] = rm
        texts = look(users, rooms, 0)
        assert texts[0] == b"\n~FTRoom: " + mark + rooms[rm]["name"] + b"\n\n" and texts[1] == b""
        assert texts[2] == b"\n~FTThere are no exits.\n\n" and texts[3:5] == [b"~FTYou are all alone here.\n", b"\n"]
        assert texts[5] == b"Access is " + words + b" and there are ~OL~FM0~RS messages on the board.\n"
        assert texts[6] == b"No topic has been set yet.\n" and len(texts) == 7
    users[0]["room"] = 0
    rooms[0].update(links=[1, 2, 3, 0, 1, 2, 3, 0, 1, 2], topic=b"t" * 60, mesg_cnt=2**31 - 1, desc=b"A room.\n")
    texts = look(users, rooms, 0)
    assert texts[2] == (b"\n~FTExits are:  ~FRpriv  ~FGfpub  ~FRfpriv  ~FGpub  ~FRpriv  ~FGfpub  ~FRfpriv  ~FGpub  ~FRpriv  ~FGfpub"
                        b"\n\n")
    assert texts[1] == b"A room.\n" and texts[6] == b"Current topic: " + b"t" * 60 + b"\n"
    assert texts[5] == b"Access is set to ~FGPUBLIC~RS and there are ~OL~FM2147483647~RS messages on the board.\n"
    rooms[0].update(netlink=(b"peer", True))
    assert look(users, rooms, 0)[2].endswith(b"  ~FGfpub  ~FRpeer*\n\n")
    rooms[0].update(links=[], netlink=(b"peer", False))                 # a netlink alone: no "no exits"
    assert look(users, rooms, 0)[2] == b"\n~FTExits are:  ~FGpeer*\n\n"
    # an empty description is a write_user of an empty string: no write without colour, the reset alone with it
    assert nuts_path.chunks(b"", 0) == [] and nuts_path.chunks(b"", 1) == [b"\x1b[0m"]
    rooms[0].update(desc=b"")
    users[0]["colour"] = 0
    plain = model_chunks(users, rooms, 0)
    users[0]["colour"] = 1
    assert len(model_chunks(users, rooms, 0)) == 2 * len(plain) + 1 == 13


# ------------------------------------------------------------------ bounds
def test_a_member_line_stays_within_its_bounds():
    most_bytes = most_writes = longest = 0
    for name, desc, vis, afk in itertools.product(WORST_NAMES, WORST_DESCS + (b"\n" * 29 + b"/",), (0, 1), (0, 1)):
        line = member_line(look_user(1, name=name, desc=desc, vis=vis, afk=afk))
        longest = max(longest, len(line))
        for c in (0, 1):
            ch = nuts_path.chunks(line, c)
            most_bytes, most_writes = max(most_bytes, sum(map(len, ch))), max(most_writes, len(ch))
            assert sum(map(len, ch)) <= device.MAX_MEMBER_BYTES and len(ch) <= device.MAX_MEMBER_WRITES
            assert max(map(len, ch)) < 994                              # never near a flush in mid-line
    # the derivation: 42 bytes of the fixed parts with colour on, and 6 per byte of a name and a desc of newlines
    worst = member_line(look_user(1, name=b"\n" * 12, desc=b"\n" * 30, vis=0, afk=1))
    assert len(nuts_path.transduce(worst, 1)) == 42 + 6 * 42 == device.MAX_MEMBER_BYTES == most_bytes
    assert most_writes == device.MAX_MEMBER_WRITES == 2 and longest == len(worst) == device.MAX_MEMBER_LINE == 69 <= device._LINE_ROW


def test_the_room_texts_fit_their_slots_and_the_variant_bounds():
    caps = [b - a for a, b in zip(device._LOOK_TEXT_AT, device._LOOK_TEXT_AT[1:] + (device._LOOK_STRIDE,))]
    assert caps == [36, 812, 352, 96, 80] and device._LOOK_STRIDE < device.TEXT_SIZE
    rooms = [new_room(b"N" * 20, access=device.FIXED_PRIVATE, links=[0] * 10, topic=b"t" * 60, mesg_cnt=2**31 - 1,
                      netlink=(b"s" * 80, True))]
    users = {0: look_user(0, name=b"A")}
    longest = [0] * 5
    for desc in (b"\n" * 810, b"~FR" * 270, b"/~" * 405, b"d" * 810, b""):
        rooms[0]["desc"] = desc
        texts = look(users, rooms, 0)
        for i, text in enumerate(texts[:3] + texts[5:]):
            longest[i] = max(longest[i], len(text))
            assert len(text) <= caps[i] and len(text) < device.TEXT_SIZE
            for c in (0, 1):
                ch = nuts_path.chunks(text, c)
                assert sum(map(len, ch)) <= device.max_bytes(len(text)) and len(ch) <= device.MAX_WRITES
    assert longest == [35, 810, 352, 96, 76]
    for text, cap in ((b"~FTYou can see:\n", 16), (b"~FTYou are all alone here.\n", 28), (b"\n", 4)):
        assert len(text) <= cap
    assert device._LOOK_FIXED_AT == (0, 16, 44) and device._LOOK_FIXED_STRIDE == 48


# ------------------------------------------------------------------ the dataclass
def hand_built_look():
    """A Look from the model alone: texts and variants scattered over buffers of 0xAA bytes, -7 in the unused chunk sizes."""
    rooms = fuzz_rooms(__import__("random").Random(3))
    users = {0: look_user(0, name=b"Zero", room=0, colour=1), 5: look_user(5, name=b"Five", room=0, vis=0, level=3, desc=b"is five/"),
             6: look_user(6, name=b"Six", room=0, afk=1, desc=b"~FRred"), 7: look_user(7, name=None, room=0),
             9: look_user(9, name=b"Nine", room=1)}
    slots = [0, 9, 5, 0]
    order = {}
    for s in slots:
        order.setdefault(users[s]["room"], len(order))
    rms = list(order)
    line_of = {}
    for rm in rms:
        for j in sorted(users):
            if users[j]["room"] == rm and users[j]["name"]:
                line_of[j] = len(line_of)
    strings = {}
    for i, rm in enumerate(rms):
        anyone = next(j for j in users if users[j]["room"] == rm)
        texts = look(users, rooms, anyone)
        for j, t in zip(range(5), texts[:3] + texts[-2:]):
            strings[5 * i + j] = t
    fixed = 5 * len(rms)
    strings.update({fixed: b"~FTYou can see:\n", fixed + 1: b"~FTYou are all alone here.\n", fixed + 2: b"\n"})
    for j, l in line_of.items():
        strings[fixed + 3 + l] = member_line(users[j])
    T = fixed + 3 + len(line_of)
    texts, variants = np.full(8000, 0xAA, dtype=np.uint8), np.full(60_000, 0xAA, dtype=np.uint8)
    tstarts, tsizes = np.zeros(T, dtype=np.int64), np.full(T, -1, dtype=np.int64)
    starts, sizes = np.zeros((T, 2), dtype=np.int64), np.zeros((T, 2), dtype=np.int64)
    counts, wsz = np.zeros((T, 2), dtype=np.int32), np.full((T, 2, device.MAX_WRITES), -7, dtype=np.int32)
    at, vat = 3, 7
    for t, text in strings.items():
        tstarts[t], tsizes[t] = at, len(text)
        texts[at:at + len(text)] = np.frombuffer(text, dtype=np.uint8)
        at += len(text) + 5
        for c in (0, 1):
            ch = nuts_path.chunks(text, c)
            data = b"".join(ch)
            starts[t, c], sizes[t, c], counts[t, c] = vat, len(data), len(ch)
            variants[vat:vat + len(data)] = np.frombuffer(data, dtype=np.uint8)
            wsz[t, c, :len(ch)] = [len(x) for x in ch]
            vat += len(data) + 3
    listed = [members(users, s) for s in slots]
    lk = device.Look(slots=np.array(slots, dtype=np.int32), colour=np.array([users[s]["colour"] for s in slots], dtype=np.uint8),
                     room_index=np.array([order[users[s]["room"]] for s in slots], dtype=np.int32),
                     rooms=np.array(rms, dtype=np.int32), member_slots=np.array(sum(listed, []), dtype=np.int32),
                     member_lines=np.array([line_of[j] for j in sum(listed, [])], dtype=np.int32),
                     member_starts=np.cumsum([0] + [len(x) for x in listed[:-1]]).astype(np.int64),
                     member_counts=np.array([len(x) for x in listed], dtype=np.int32),
                     line_slots=np.array(sorted(line_of, key=line_of.get), dtype=np.int32), texts=texts, text_starts=tstarts,
                     text_sizes=tsizes, variants=variants, variant_starts=starts, variant_sizes=sizes, write_counts=counts,
                     write_sizes=wsz)
    return lk, users, rooms, slots


def test_a_hand_built_look_obeys_the_contract(no_library):
    lk, users, rooms, slots = hand_built_look()
    assert lk.timing == {} and lk.rooms.tolist() == [0, 1] and lk.line_slots.tolist() == [0, 5, 6, 9]
    for k, slot in enumerate(slots):
        assert lk.chunks(k) == model_chunks(users, rooms, slot) and lk.output(k) == b"".join(lk.chunks(k))
        assert lk.members(k).tolist() == members(users, slot)
        assert [lk.text(t) for t in lk.text_numbers(k)] == look(users, rooms, slot)
    assert lk.members(0).tolist() == [6] and lk.members(1).tolist() == [] and lk.members(2).tolist() == [0, 6]
    assert lk.chunks(0) == lk.chunks(3) and lk.chunks(0)[-1] == b"\x1b[0m"         # the same looker twice; colour on
    assert b"You are all alone here." in lk.output(1) and b"(AFK)" in lk.output(2) and b"\x1b" not in lk.output(2)
    for bad_k in (-1, 4):
        for call in (lk.chunks, lk.output, lk.members, lk.text_numbers):
            with pytest.raises(IndexError):
                call(bad_k)


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def look_run(built):
    res = child_run.run_child("device_look_child.py", "DEVICE_LOOK", 600)
    print("\n[look]", json.dumps(res)[:4000])
    return res


@pytest.mark.gpu
def test_the_golden_sessions_replay_on_the_device(look_run):
    g = look_run["golden"]
    assert list(g) == list(GOLDEN)
    for name in GOLDEN:
        assert g[name]["compared"] == golden_looks(name), name
        assert g[name]["mismatches"] == [] and g[name]["n_bad_vs_model"] == 0, (name, g[name])
    assert sum(g[name]["compared"] for name in GOLDEN) == 49


@pytest.mark.gpu
def test_seeded_looks_match_the_model(look_run):
    f = look_run["fuzz"]
    assert f["capacities"] == list(CAPACITIES) == [1, 63, 64, 65, 255, 256, 257, 1000]
    assert f["calls"] == 2 * len(CAPACITIES) and f["looks"] == f["calls"] * LOOKERS_PER_CALL and LOOKERS_PER_CALL == 64
    assert f["access"] == [0, 1, 2, 3] and f["colours"] == [0, 1]
    assert f["hidden_by_level"] > 0 and f["afk"] > 0 and f["alone"] > 0 and f["most_members"] > 256
    assert f["n_bad"] == 0, f["first_bad"]


@pytest.mark.gpu
def test_the_texts_are_the_models_and_their_variants_plan_manys(look_run):
    c = look_run["contract"]
    assert c["checked"] >= 40 and c["room_texts"] >= 15
    assert c["n_bad"] == 0, c["first_bad"]


@pytest.mark.gpu
def test_a_second_run_gives_identical_bytes(look_run):
    assert look_run["determinism"] == {"same_on_a_second_call": True, "same_on_a_second_roster": True}


@pytest.mark.gpu
def test_nothing_else_moved(look_run):
    m = look_run["moved"]
    assert m["with_look_rooms"] == m["fresh"]                           # results and copy volumes alike
    # ... and after look_many calls the other calls still return what they return on the fresh roster; a call may copy
    # less there, never more: a look call that found the allocation grown has uploaded the table again already
    for call, parts in m["fresh_again"].items():
        assert m["after_looking"][call][:-1] == parts[:-1], call
        assert all(x <= y for x, y in zip(m["after_looking"][call][-1], parts[-1])), call
    h, cap, rooms = m["look_h2d"], m["capacity"], m["look_rooms"]
    # clean tables: the lookers, their rooms, the ranges and the texts' offsets alone -- five small arrays in a 256-byte
    # slice each, 4 bytes per text (five per room, three fixed, a line per slot of the two rooms) and the violation count
    assert len(set(h["clean"] + [h["clean_again"]])) == 1
    assert h["clean"][0] == 5 * 256 + -(-4 * (5 * 2 + 3 + cap) // 256) * 256 + 4 < 32 * cap
    # the descriptions' upload is 32 bytes per slot rounded up to a 256-byte slice: the slack is below 256 bytes
    assert 32 * cap <= h["after_desc_update"] - h["clean"][0] < 32 * cap + 256
    # the room table lies in front of the descriptions, so they travel with it: two slices, below 512 bytes of slack
    assert 1072 * rooms + 32 * cap <= h["after_set_rooms"] - h["clean"][0] < 1072 * rooms + 32 * cap + 512
    assert h["first"] > h["after_set_rooms"]                            # the table and the speaker state as well
