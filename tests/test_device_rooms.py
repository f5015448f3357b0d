"""``Roster.rooms_many``: rooms() -- ``.rmst`` and ``.rmsn`` -- composed over the roster on the device
(nuts_roster_rooms_count and nuts_roster_rooms_lines of fanout.hip), ``device.Rooms``, and the three netlink facts
``.rmsn`` prints, kept in the room record's flag byte (``Roster.set_rooms(inlink=, netlink=)``).

Host tier (unmarked): everything malformed is rejected before the device library loads, and a rejected call changes no
mirror and no dirty flag; the room record byte for byte; the Python model of ``rooms()`` (``rooms`` of
tests/device_rooms_child.py) reproduces every listing of the recorded session tests/golden/reference_only/rmst.json,
through the CPU restatement's transducer; the rules of the count and of the line on hand-built rosters; the longest lines
stay within their bounds on the CPU restatement; a ``Rooms`` built by hand obeys its contract; and over a library that
computes nothing, ``rooms_many`` is passed exactly the mirrors it reads whose flags were set, also interleaved with the
other calls.  In the recorded session a link is DOWN or absent and inlink is YES and NO; the UP and VER states are tested
against the model only.  The kernels' scratch-free compile is tests/test_device_fanout.py's, which looks at every
function of fanout.hip.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_rooms_child.py, under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import json
import re
from pathlib import Path

import numpy as np
import pytest

import child_run
from device_look_child import look_user
from device_rooms_child import (CAPACITIES, HEAD_LINKS, HEAD_TOPICS, LOOK_ROOMS, LOOKERS_PER_CALL, cases, counted, golden_listings,
                                list_room, model_chunks, replay_listings, room_line, rooms, set_rooms, worst_rooms, COMMANDS)
from nuts333_amd import device, nuts_path

REPO = Path(__file__).resolve().parent.parent
FLAGS = ("_dirty", "_speech_dirty", "_private_dirty", "_afk_dirty", "_rooms_dirty", "_udesc_dirty", "_who_dirty", "_clones_dirty")
MIRRORS = ("_table", "_speech", "_rooms", "_udesc", "_who", "_afk", "_clones")


def flags(r):
    return tuple(getattr(r, f) for f in FLAGS)


def clean(r):
    for f in FLAGS:
        setattr(r, f, False)


def mirrors(r):
    return [getattr(r, m).copy() for m in MIRRORS]


def hand_rooms() -> list:
    return [list_room(b"drive", access=device.FIXED_PUBLIC), list_room(b"corridor", netlink=(b"faraway", False, device.LINK_DOWN)),
            list_room(b"lounge", inlink=True), list_room(b"up", netlink=(b"srv", True))]


def seated(capacity=6, **kw) -> device.Roster:
    """A roster over hand_rooms() whose slots 0 and 1 stand in room 0."""
    rms = hand_rooms()
    r = device.Roster(capacity, look_rooms=len(rms), **kw)
    set_rooms(r, rms)
    r.update([0, 1], room=0, name=[b"Alice", "Bobby"])
    return r


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


# ------------------------------------------------------------------ host tier: names and input checks
def test_the_new_names_exist():
    assert len(device.KERNELS) == 18 and device.KERNELS[-1] == "nuts_roster_look"         # unchanged
    assert device.WHO_KERNELS == ("nuts_roster_who", "nuts_roster_who_shown")
    assert device.ROOMS_KERNELS == ("nuts_roster_rooms_count", "nuts_roster_rooms_lines")
    assert not set(device.ROOMS_KERNELS) & (set(device.KERNELS) | set(device.WHO_KERNELS))
    source = device.SOURCE.read_text()
    for k in device.ROOMS_KERNELS:
        assert f"{k}(RoomsArgs a)" in source
    assert (device.COM_RMST, device.COM_RMSN) == (42, 43)
    assert (device.ROOMS_HEAD_TOPICS, device.ROOMS_HEAD_LINKS, device.ROOMS_TAIL) == (0, 1, 2)
    assert (device.LINK_DOWN, device.LINK_VERIFYING, device.LINK_UP) == (0, 1, 2)
    assert (device.MAX_RMST_LINE, device.MAX_RMSN_LINE) == (121, 162)
    assert device.MAX_RMST_LINE <= device._RMST_ROW == 124 and device.MAX_RMSN_LINE <= device._RMSN_ROW == 164 < device.TEXT_SIZE
    assert callable(device.Roster.rooms_many) and device.Rooms.__dataclass_fields__.keys() >= {"slots", "colour", "topics", "counts"}
    assert "constexpr int kRmstRow = 124, kRmsnRow = 164;" in source and "kRmstLineMax == 121 && kRmsnLineMax == 162" in source


@pytest.mark.parametrize("slots", [[], (), None, 3, "01", b"01"])
def test_slots_must_be_a_non_empty_sequence(no_library, slots):
    r = seated()
    clean(r)
    with pytest.raises(ValueError, match="slots|empty call"):
        r.rooms_many(slots, topics=True)
    assert flags(r) == (False,) * len(FLAGS)


def test_a_bad_slot_is_named_by_its_position(no_library):
    r = seated()
    for bad, why in (([0, 6], "rooms 1: slot"), ([0, 1, -1], "rooms 2: slot"), ([None], "rooms 0: slot"), ([True], "rooms 0: slot"),
                     ([0.0], "rooms 0: slot")):
        with pytest.raises(ValueError, match=why):
            r.rooms_many(bad, topics=False)


@pytest.mark.parametrize("topics, why", [
    (1, "topics must be a bool"), (None, "topics must be a bool"), ("yes", "topics must be a bool"), (b"\1", "topics must be a bool"),
    ([True], "1 values for 2 lookers"), ([True, False, True], "3 values for 2 lookers"), ([], "0 values for 2 lookers"),
    ([True, 1], "rooms 1: topics must be a bool"), ([None, False], "rooms 0: topics must be a bool"),
])
def test_topics_is_a_bool_or_one_per_looker(no_library, topics, why):
    r = seated()
    clean(r)
    before = mirrors(r)
    with pytest.raises(ValueError, match=why):
        r.rooms_many([0, 1], topics=topics)
    assert flags(r) == (False,) * len(FLAGS) and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))


def test_topics_is_keyword_only_and_required(no_library):
    with pytest.raises(TypeError):
        seated().rooms_many([0], True)
    with pytest.raises(TypeError):
        seated().rooms_many([0])


def test_a_roster_without_room_records_a_closed_one_and_a_call_past_the_cap(no_library, monkeypatch):
    r = device.Roster(4)
    r.update(0, room=0, name=b"Alice")
    state = flags(r)
    with pytest.raises(ValueError, match=r"no room records \(look_rooms is 0\)"):
        r.rooms_many([0], topics=True)
    assert flags(r) == state
    r = seated()
    state, before = flags(r), mirrors(r)
    ctext = 180 + 4 * (124 + 164)
    monkeypatch.setattr(device, "MANY_ARENA_CAP", 12 * ctext + 16 * 11 + 4 * 4 - 1)
    with pytest.raises(ValueError, match=f"call too large: its variant and count bound is {12 * ctext + 16 * 11 + 16} bytes.*MANY_ARENA_CAP.*split it"):
        r.rooms_many([0], topics=True)
    assert flags(r) == state and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))
    r.close()
    with pytest.raises(ValueError, match="closed"):
        r.rooms_many([0], topics=True)
    with pytest.raises(ValueError, match="closed"):
        r.set_rooms(0, inlink=True)


# ------------------------------------------------------------------ host tier: set_rooms
def test_a_record_without_the_new_fields_is_todays(no_library):
    r = device.Roster(2, look_rooms=3)
    r.set_rooms([0, 1, 2], name=[b"a", b"b", b"c"], netlink=[None, (b"srv", False), (b"in", True)])
    assert r._room_rec[:, 24].tolist() == [0, 1, 3]                     # 1: UP, 2: allow_in -- as before the new bits
    assert r._room_rec[1, 132:135].tobytes() == b"srv" and r._room_rec[1, 25] == 3
    explicit = device.Roster(2, look_rooms=3)
    explicit.set_rooms([0, 1, 2], name=[b"a", b"b", b"c"], inlink=False,
                       netlink=[None, (b"srv", False, device.LINK_UP), (b"in", True, device.LINK_UP)])
    assert np.array_equal(explicit._rooms, r._rooms)


def test_the_flag_byte(no_library):
    r = device.Roster(2, look_rooms=4)
    clean(r)
    r.set_rooms([0, 1, 2], netlink=[(b"d", False, device.LINK_DOWN), (b"v", True, device.LINK_VERIFYING), (b"u", True, device.LINK_UP)])
    assert r._room_rec[:, 24].tolist() == [8, 16 | 2, 1 | 2, 0]
    assert flags(r) == tuple(f == "_rooms_dirty" for f in FLAGS)
    clean(r)
    r.set_rooms([0, 3], inlink=True)
    assert r._room_rec[:, 24].tolist() == [8 | 4, 16 | 2, 1 | 2, 4] and flags(r) == tuple(f == "_rooms_dirty" for f in FLAGS)
    r.set_rooms([0, 3], netlink=[(b"u", False), None])                  # netlink= keeps the inlink bit
    assert r._room_rec[:, 24].tolist() == [1 | 4, 16 | 2, 1 | 2, 4]
    r.set_rooms(0, netlink=None)
    assert r._room_rec[0, 24] == 4 and r._room_rec[0, 25] == 0 and not r._room_rec[0, 132:212].any()
    r.set_rooms([1, 1, 3, 3], inlink=[True, False, False, True],        # the last value of a room given twice wins
                netlink=[None, (b"late", False, device.LINK_DOWN), (b"x", True), None])
    assert r._room_rec[:, 24].tolist() == [4, 8, 1 | 2, 4] and r._room_rec[1, 132:136].tobytes() == b"late"
    r.set_rooms(1, inlink=np.bool_(True))
    assert r._room_rec[1, 24] == 8 | 4


@pytest.mark.parametrize("fields, why", [
    ({"inlink": 1}, "room 0: inlink must be a bool"), ({"inlink": None}, "inlink must be a bool"), ({"inlink": "yes"}, "inlink"),
    ({"inlink": [True]}, "1 values for 2 rooms"), ({"inlink": [True, 0]}, "room 1: inlink must be a bool"),
    ({"netlink": (b"s", True, 3)}, "state must be LINK_DOWN"), ({"netlink": (b"s", True, -1)}, "state must be LINK_DOWN"),
    ({"netlink": (b"s", True, True)}, "state must be LINK_DOWN"), ({"netlink": (b"s", True, None)}, "state must be LINK_DOWN"),
    ({"netlink": (b"s", True, 1.0)}, "state must be LINK_DOWN"), ({"netlink": (b"s", 1, device.LINK_UP)}, "netlink must be None or"),
    ({"netlink": (b"s", True, 0, 0)}, "netlink"), ({"netlink": [(b"s", True, 0), (b"t", True, 9)]}, "room 1: a netlink's state"),
    ({"inlink": True, "netlink": (b"s" * 81, True, 0)}, "netlink service"), ({"inlink": True, "mesg_cnt": -1}, "mesg_cnt"),
])
def test_a_rejected_set_rooms_changes_nothing(no_library, fields, why):
    r = seated()
    clean(r)
    before = mirrors(r)
    with pytest.raises(ValueError, match=why):
        r.set_rooms([1, 2], **fields)
    assert flags(r) == (False,) * len(FLAGS) and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))


def test_only_a_link_that_is_up_can_be_away_over(no_library):
    r = seated()
    r.set_rooms([1, 2, 3], netlink=[(b"d", False, device.LINK_DOWN), (b"v", False, device.LINK_VERIFYING), (b"u", False, device.LINK_UP)])
    for room in (0, 1, 2):
        with pytest.raises(ValueError, match=f"room {room} has no netlink"):
            r.update(2, away=room)
    r.update(2, away=3)
    assert r._who[2, 1] == 3


# ------------------------------------------------------------------ host tier: the model
def test_the_model_reproduces_the_recorded_session():
    res = replay_listings(lambda users, rms, slot, line: b"".join(model_chunks(users, rms, slot, COMMANDS[line][1])))
    assert res["mismatches"] == [] and res["compared"] == golden_listings() == 9
    assert res["kinds"] == {"rmst_colour": 2, "rmst_plain": 3, "rmsn_colour": 2, "rmsn_plain": 2}
    doc = json.loads((REPO / "tests" / "golden" / "reference_only" / "rmst.json").read_text())
    steps = [s for s in doc["steps"] if s.get("send") in COMMANDS]
    text = "".join(s["recv"][s["actor"]] for s in steps)
    # what the session claims to hold: the fixed rooms' star before a colour command, a room made private in red and
    # plain, a message on a board, the topic with its colour command rendered and stripped, a link that is down with its
    # service, an inlink, and a room with neither
    for needle in (" *\x1b[31mPRIV", " * \x1b[32mPUB", "corridor             :   \x1b[31mPRIV\x1b[0m      1", "corridor             :   PRIV      1",
                   "      2      1  a \x1b[32mgreen\x1b[0m topic", "      3      1  a green topic", "     NO   DOWN  faraway",
                   "    YES   \x1b[31mDOWN\x1b[0m  \x1b[0m", "     NO      -  \n"):
        assert needle in text, needle
    by_send = [s["send"] for s in doc["steps"] if "send" in s]
    assert {".topic a ~FGgreen~RS topic", ".write one line on the board", ".private", ".clone hallway", ".invis", ".go hallway"} <= set(by_send)
    assert sum(s["op"] == "connect" for s in doc["steps"]) == 5 and sum(s["op"] == "login" for s in doc["steps"]) == 4
    # the invisible user is counted and the clone and the name prompt are not: four logins, always four users in all
    last = steps[-1]["recv"][steps[-1]["actor"]]
    assert [int(re.search(r"(?:PUB|PRIV) +(\d+) +\d+ ", l).group(1)) for l in last.split("\n\r")[5:10]] == [2, 1, 0, 1, 0]
    assert {a["level"] for a in doc["accounts"][0]} == {0, 1, 2, 3} and sum(a["colour"] for a in doc["accounts"][0]) == 1


def hand_users() -> dict:
    return {0: look_user(0, name=b"Zero", room=0, colour=1), 1: look_user(1, name=b"Hidden", room=0, vis=0, level=4),
            2: look_user(2, name=None, room=0),                         # no user
            3: look_user(3, name=b"Prompt", room=0, login=1),           # at login stage, with a room: a clone's seat in the replayer
            4: look_user(4, name=b"Away", room=None),                   # roomless
            5: look_user(5, name=b"Far", room=4),                       # a room at or past look_rooms
            6: look_user(6, name=b"Lounger", room=2), 7: look_user(7, name=None, room=None, login=1)}


def test_who_is_counted():
    users, rms = hand_users(), hand_rooms()
    assert [counted(users, r) for r in range(4)] == [2, 0, 1, 0]       # the invisible one counts
    assert rooms(users, rms, True) == [HEAD_TOPICS, b"drive                :  * ~FGPUB~RS      2      0  \n",
                                       b"corridor             :    ~FGPUB~RS      0      0  \n",
                                       b"lounge               :    ~FGPUB~RS      1      0  \n",
                                       b"up                   :    ~FGPUB~RS      0      0  \n", b"\n"]
    assert rooms(users, rms, False) == [HEAD_LINKS, b"drive                :  * ~FGPUB~RS      2      0      NO      -~RS  \n",
                                        b"corridor             :    ~FGPUB~RS      0      0      NO   ~FRDOWN~RS  faraway\n",
                                        b"lounge               :    ~FGPUB~RS      1      0     YES   ~FRDOWN~RS  \n",
                                        b"up                   :    ~FGPUB~RS      0      0      NO     ~FGUP~RS  srv\n", b"\n"]


def test_the_lines_fields():
    line = lambda topics=True, count=0, **f: room_line(list_room(**{"name": b"r", **f}), count, topics)
    front = b"r" + b" " * 19 + b" : "
    # %9s over an 8-byte string, with and without the star
    assert line(access=device.PUBLIC).startswith(front + b"   ~FGPUB~RS") and line(access=device.FIXED_PUBLIC).startswith(front + b" * ~FGPUB~RS")
    assert line(access=device.PRIVATE).startswith(front + b"  ~FRPRIV~RS") and line(access=device.FIXED_PRIVATE).startswith(front + b" *~FRPRIV~RS")
    # %3d widens
    for count, digits in ((0, b"  0"), (9, b"  9"), (99, b" 99"), (999, b"999"), (1000, b"1000"), (65536, b"65536")):
        assert line(count=count) == front + b"   ~FGPUB~RS    " + digits + b"      0  \n"
    assert line(mesg_cnt=2**31 - 1).endswith(b"~RS      0    2147483647  \n") and line(mesg_cnt=100).endswith(b"      0    100  \n")
    assert line(name=b"n" * 20).startswith(b"n" * 20 + b" : ") and line(name=b"exactly_twenty_bytes").index(b" : ") == 20
    colours = b"~FR~FG~FB~FT~OL~UL~RS~LI~RV~FK~FY~FM~FW~BK~BR~BG~BY~BB~BM~BT"
    assert len(colours) == 60 and line(topic=colours).endswith(b"  " + colours + b"\n")
    assert nuts_path.transduce(line(topic=colours), 0).endswith(b"      0  \n\r")             # all of it is commands
    serv = b"s" * 80
    # all four stat strings, and NO / YES; the service whenever there is a netlink
    tail = lambda **f: line(False, **f).split(b"      0      0", 1)[1]
    assert tail() == b"      NO      -~RS  \n" and tail(inlink=True) == b"     YES   ~FRDOWN~RS  \n"
    assert tail(netlink=(serv, False, device.LINK_DOWN)) == b"      NO   ~FRDOWN~RS  " + serv + b"\n"
    assert tail(netlink=(serv, True, device.LINK_UP), inlink=True) == b"     YES     ~FGUP~RS  " + serv + b"\n"
    assert tail(netlink=(b"", True, device.LINK_VERIFYING)) == b"      NO    ~FYVER~RS  \n"
    assert tail(netlink=(b"two", False)) == b"      NO     ~FGUP~RS  two\n"                 # today's 2-tuple is a link that is UP


def test_a_nameless_room_is_skipped_and_an_empty_talker():
    rms = [list_room(b"a"), list_room(b"", topic=b"unseen"), list_room(b"c")]
    users = {0: look_user(0, name=b"A", room=1)}
    assert [s[:1] for s in rooms(users, rms, True)] == [b"\n", b"a", b"c", b"\n"] and len(rooms(users, rms, False)) == 4
    assert rooms({0: look_user(0, name=None, room=None, login=1)}, [list_room(b"")], True) == [HEAD_TOPICS, b"\n"]
    assert rooms({}, [list_room(b"only")], False) == [HEAD_LINKS, b"only                 :    ~FGPUB~RS      0      0      NO      -~RS  \n", b"\n"]


def test_the_longest_lines_stay_within_their_bounds():
    """121 and 162 bytes, from the formats; through the transducer at most 6 bytes a byte and the reset, and one write and
    the reset's: a line of 162 newlines would be 976 bytes, below the 995 at which the staging buffer is flushed."""
    assert (device.MAX_RMST_LINE_BYTES, device.MAX_RMSN_LINE_BYTES, device.MAX_ROOMS_LINE_WRITES) == (730, 976, 2)
    assert device.MAX_RMSN_LINE_BYTES == device.max_bytes(device.MAX_RMSN_LINE) and device.MAX_RMST_LINE_BYTES == device.max_bytes(device.MAX_RMST_LINE)
    longest = {True: 0, False: 0}
    for rm in worst_rooms():
        for topics, most in ((True, device.MAX_RMST_LINE_BYTES), (False, device.MAX_RMSN_LINE_BYTES)):
            line = room_line(rm, 65536, topics)
            longest[topics] = max(longest[topics], len(line))
            for c in (0, 1):
                ch = nuts_path.chunks(line, c)
                assert sum(map(len, ch)) <= most and len(ch) <= device.MAX_ROOMS_LINE_WRITES
    assert longest == {True: device.MAX_RMST_LINE, False: device.MAX_RMSN_LINE} == {True: 121, False: 162}
    gaps = [b - a for a, b in zip(device._ROOMS_FIXED_AT, device._ROOMS_FIXED_AT[1:] + (device._ROOMS_FIXED_STRIDE,))]
    assert [len(HEAD_TOPICS), len(HEAD_LINKS), 1] == [79, 96, 1] and all(n <= g for n, g in zip([79, 96, 1], gaps))
    assert HEAD_TOPICS.startswith(b"\n~BB*** Rooms data ***\n\n~FTRoom name            : Access  Users  Mesgs  ")


# ------------------------------------------------------------------ the dataclass
def hand_built_rooms(kinds=(True, False, False, True)):
    """A Rooms from the model alone: texts and variants scattered over buffers of 0xAA bytes, -7 in the unused chunk sizes."""
    users, rms = hand_users(), hand_rooms() + [list_room(b"", topic=b"nameless")]
    nr, slots = len(rms), [0, 1, 6, 0]
    strings = {device.ROOMS_TAIL: b"\n"}
    for topics, head, first in ((True, 0, 3), (False, 1, 3 + nr)):
        if topics in kinds:
            strings[head] = HEAD_TOPICS if topics else HEAD_LINKS
            strings.update({first + r: room_line(rm, counted(users, r), topics) for r, rm in enumerate(rms) if rm["name"]})
    T = 3 + 2 * nr
    texts, variants = np.full(4000, 0xAA, dtype=np.uint8), np.full(20_000, 0xAA, dtype=np.uint8)
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
    got = device.Rooms(slots=np.array(slots, dtype=np.int32), colour=np.array([users[s]["colour"] for s in slots], dtype=np.uint8),
                       topics=np.array(kinds, dtype=np.uint8), counts=np.array([counted(users, r) for r in range(nr)], dtype=np.int32),
                       texts=texts, text_starts=tstarts, text_sizes=tsizes, variants=variants, variant_starts=starts,
                       variant_sizes=sizes, write_counts=counts, write_sizes=wsz)
    return got, users, rms, slots


def test_a_hand_built_rooms_obeys_the_contract(no_library):
    got, users, rms, slots = hand_built_rooms()
    nr = len(rms)
    assert got.timing == {} and got.counts.tolist() == [2, 0, 1, 0, 1]  # a nameless room is counted, and not listed
    for k, (slot, topics) in enumerate(zip(slots, (True, False, False, True))):
        assert got.chunks(k) == model_chunks(users, rms, slot, topics) and got.output(k) == b"".join(got.chunks(k))
        assert [got.text(t) for t in got.text_numbers(k)] == rooms(users, rms, topics)
    assert got.text_numbers(0) == [device.ROOMS_HEAD_TOPICS, 3, 4, 5, 6, device.ROOMS_TAIL]  # room 4 has no name
    assert got.text_numbers(1) == [device.ROOMS_HEAD_LINKS, 3 + nr, 4 + nr, 5 + nr, 6 + nr, device.ROOMS_TAIL]
    assert got.chunks(0) == got.chunks(3) and got.chunks(0)[-1] == b"\x1b[0m" and b"\x1b" not in got.output(1)
    for bad_k in (-1, 4):
        for call in (got.chunks, got.output, got.text_numbers):
            with pytest.raises(IndexError):
                call(bad_k)
    for bad_t in (-1, 3 + 2 * nr, 3 + 4, 3 + nr + 4):                   # past the texts; the nameless room's lines
        with pytest.raises(IndexError):
            got.text(bad_t)
    for bad_t in (-1, 3 + 2 * nr):
        with pytest.raises(IndexError):
            got.text_chunks(bad_t, 0)
    with pytest.raises(IndexError):
        got.text_chunks(0, 2)
    only, users, rms, slots = hand_built_rooms(kinds=(True, True, True, True))               # a kind nobody asks for is void
    assert only.text_sizes[device.ROOMS_HEAD_LINKS] == -1 and (only.text_sizes[3 + nr:] == -1).all()
    assert only.text_chunks(device.ROOMS_HEAD_LINKS, 1) == [] and only.text_numbers(2)[0] == device.ROOMS_HEAD_TOPICS
    with pytest.raises(IndexError):
        only.text(device.ROOMS_HEAD_LINKS)


# ------------------------------------------------------------------ dirty flags, over a library that computes nothing
ROOMS_MIRROR_ARGS = dict(zip(range(4, 7), ("_table", "_speech", "_rooms")))


class FakeLibrary:
    """Every ``nd_roster_*`` call returns 0 and is kept in ``calls`` as ``(name, args)``."""

    def __init__(self, arrays: dict):
        self.calls, self.arrays = [], arrays
        self._buffer = np.zeros(16, dtype=np.uint8)

    def nd_arena(self):
        return self._buffer.ctypes.data

    nd_write_sizes = nd_arena

    def nd_last_error(self):
        return b"the fake library has no errors"

    def __getattr__(self, name):
        if not name.startswith("nd_roster_"):
            raise AttributeError(name)

        def call(*args):
            if name in ("nd_roster_create", "nd_roster_destroy", "nd_roster_review_rooms", "nd_roster_revtell_rings",
                        "nd_roster_look_rooms", "nd_roster_clones"):
                return 0
            self.calls.append((name, args))
            if name == "nd_roster_tell":                                # tell_many indexes by what the device found
                self.arrays[args[15]][:] = -1
                self.arrays[args[16]][:] = -1
            return 0
        return call


@pytest.fixture
def fake(monkeypatch):
    arrays: dict = {}
    lib = FakeLibrary(arrays)
    real = device._ptr

    def ptr(a):
        arrays[a.ctypes.data] = a
        return real(a)

    monkeypatch.setattr(device, "_ptr", ptr)
    monkeypatch.setattr(device, "_load", lambda: lib)
    return lib


def passed(lib, r) -> set:
    """The mirrors of ``r`` the last library call was handed."""
    name, args = lib.calls[-1]
    ints = {a for a in args if isinstance(a, int) and not isinstance(a, bool)}
    return {m for m in MIRRORS if getattr(r, m).size and getattr(r, m).ctypes.data in ints}


def test_rooms_many_is_passed_exactly_the_dirty_mirrors_it_reads(fake):
    r = seated(8, clones=2, review_rooms=2)
    got = r.rooms_many([0, 1, 0], topics=[True, False, True])
    name, args = fake.calls[-1]
    assert name == "nd_roster_rooms" and args[1] == 3 and args[3] == 3 and len(args) == 15
    assert all(args[i] == getattr(r, m).ctypes.data for i, m in ROOMS_MIRROR_ARGS.items())
    # the descriptions, the login times, the AFK messages and the clone records are not rooms_many's to upload or to clear
    assert flags(r) == tuple(f in ("_afk_dirty", "_udesc_dirty", "_who_dirty", "_clones_dirty") for f in FLAGS)
    assert got.topics.tolist() == [1, 0, 1] and got.topics.dtype == np.uint8 and len(got.text_sizes) == 3 + 2 * 4 and got.counts.shape == (4,)
    r.rooms_many([0], topics=True)
    assert passed(fake, r) == set() and fake.calls[-1][1][3] == 1
    r.rooms_many([0, 1], topics=False)
    assert fake.calls[-1][1][3] == 2
    for fields, want in (({"login": 1}, {"_table"}), ({"room": 1}, {"_table"}), ({"colour": 1}, {"_table"}), ({"name": b"Zed"}, {"_speech"}),
                         ({"vis": 0}, {"_speech"}), ({"level": 3}, {"_speech"}), ({"desc": b"d"}, set()), ({"last_login": 3}, set()),
                         ({"afk_mesg": b"brb"}, set()), ({"afk": 1}, set()), ({"room": 2, "name": b"Yo", "desc": b"e"}, {"_table", "_speech"})):
        r.update(1, **fields)
        r.rooms_many([0], topics=True)
        assert passed(fake, r) == want, fields
        r.rooms_many([0], topics=True)
        assert passed(fake, r) == set(), fields
    assert r._udesc_dirty and r._who_dirty and r._afk_dirty and r._clones_dirty             # left for the calls that read them
    r.update(1, igntell=1)
    r.rooms_many([0], topics=True)
    assert passed(fake, r) == set() and r._private_dirty                # tell_many's to upload: rooms_many reads neither flag
    r.update(1, afk=1, name=b"Both")                                    # the whole speaker mirror goes up: both of its flags clear
    r.rooms_many([0], topics=True)
    assert passed(fake, r) == {"_speech"} and not r._private_dirty and not r._speech_dirty
    for fields in ({"name": b"renamed"}, {"inlink": True}, {"netlink": (b"s", False, device.LINK_DOWN)}, {"mesg_cnt": 4}, {"topic": b"t"}):
        r.set_rooms(2, **fields)
        r.rooms_many([0], topics=False)
        assert passed(fake, r) == {"_rooms"} and not r._rooms_dirty, fields
    r.set_clones(0, owner=0, room=0, hear=2)
    r.rooms_many([0], topics=True)
    assert passed(fake, r) == set() and r._clones_dirty


def test_rooms_many_interleaved_with_the_other_calls(fake):
    """No call reads a stale field, and no existing call is passed more than on a roster that never saw a rooms_many."""
    def build():
        r = seated(8, clones=2, review_rooms=2, revtell=True)
        r.set_rooms(3, netlink=(b"srv", True))
        r.set_clones(0, owner=0, room=0, hear=2)
        return r

    calls = {"look": lambda r: r.look_many([0, 1]), "relay": lambda r: r.relay_many([(b"hi\n", 0, 1, 0, 3)]),
             "tell": lambda r: r.tell_many([(0, device.COM_TELL, b"bobby psst", 3)]),
             "speak": lambda r: r.speak_many([(0, device.COM_SAY, b"hello", 1)]),
             "who": lambda r: r.who_many([0, 1], now=5, date=b"DATE"),
             "rooms": lambda r: r.rooms_many([0, 1], topics=[True, False])}
    reads = {"look": {"_table", "_speech", "_rooms", "_udesc"}, "relay": {"_table", "_clones"}, "tell": {"_table", "_speech", "_afk"},
             "speak": {"_table", "_speech"}, "who": {"_table", "_speech", "_rooms", "_udesc", "_who"}, "rooms": {"_table", "_speech", "_rooms"}}
    updates = (({"last_login": 9}, {"_who"}), ({"desc": b"new"}, {"_udesc"}), ({"vis": 0}, {"_speech"}), ({"name": b"Nom"}, {"_speech"}),
               ({"room": 1}, {"_table"}), ({"login": 0}, {"_table"}), ({"afk_mesg": b"brb"}, {"_afk"}), ({"topic": b"t"}, {"_rooms"}),
               ({"inlink": True}, {"_rooms"}))
    order = ["rooms", "look", "rooms", "relay", "tell", "who", "rooms", "speak", "look", "rooms", "tell", "relay", "who", "speak"]
    with_rooms, without = build(), build()
    for r in (with_rooms, without):
        stale, handed = set(MIRRORS), {}
        for n, (fields, which) in enumerate(updates * 3):
            if which == {"_rooms"}:
                r.set_rooms(n % 3, **fields)
            else:
                r.update(n % 2, **fields)
            stale |= which
            for kind in [k for k in order[n % 5:] + order[:n % 5] if r is with_rooms or k != "rooms"]:
                calls[kind](r)
                got = passed(fake, r)
                assert got <= stale and not (reads[kind] - got) & stale, (n, kind, got, stale)
                assert kind != "rooms" or got <= reads["rooms"]
                stale -= got
                if kind != "rooms":
                    handed[kind] = handed.get(kind, 0) + sum(getattr(r, m).nbytes for m in got)
        r.volume = handed
    assert all(with_rooms.volume[k] <= without.volume[k] for k in without.volume)
    # the room table is one mirror for look_many, who_many and rooms_many: whoever uploads it clears the flag for all three
    for first in calls.keys() & {"look", "who", "rooms"}:
        r = build()
        calls[first](r)
        assert "_rooms" in passed(fake, r) and not r._rooms_dirty
        for other in ("look", "who", "rooms"):
            calls[other](r)
            assert "_rooms" not in passed(fake, r), (first, other)
        r.set_rooms(0, inlink=True)
        calls[first](r)
        assert "_rooms" in passed(fake, r), first


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def rooms_run(built):
    res = child_run.run_child("device_rooms_child.py", "DEVICE_ROOMS", 300)
    print("\n[rooms]", json.dumps(res)[:4000])
    return res


@pytest.mark.gpu
def test_the_recorded_session_replays_on_the_device(rooms_run):
    g = rooms_run["golden"]
    assert g["compared"] == golden_listings() == 9 and g["kinds"] == {"rmst_colour": 2, "rmst_plain": 3, "rmsn_colour": 2, "rmsn_plain": 2}
    assert g["dispatched"] == [[device.COMMAND, device.COM_RMST], [device.COMMAND, device.COM_RMSN]]     # input_many hands them back
    assert g["mismatches"] == [] and g["n_bad_vs_model"] == 0, g


@pytest.mark.gpu
def test_seeded_listings_match_the_model(rooms_run):
    f = rooms_run["fuzz"]
    assert f["capacities"] == list(CAPACITIES) == [1, 64, 65, 257, 1025] and f["look_rooms"] == list(LOOK_ROOMS) == [1, 2, 64, 65, 1024]
    assert LOOKERS_PER_CALL == 8 and f["calls"] == len(cases()) == 27 and f["one_kind_calls"] >= 4 and f["colours"] == [0, 1]
    assert f["empty"] > 0 and f["single"] > 0 and f["all"] > 0 and f["uncounted"] > 0 and f["nameless_rooms"] > 0 and f["fixed"] > 0
    assert f["states"] == sorted(["None", "0", "1", "2"]) and f["inlinks"] == [False, True]
    assert f["n_bad"] == 0, f["first_bad"]


@pytest.mark.gpu
def test_the_counts_widen_the_line(rooms_run):
    w = rooms_run["widening"]
    assert w["before"]["counts"] == w["before"]["model_counts"] == [65536, 0]
    assert w["after"]["counts"] == w["after"]["model_counts"] == [65535, 1]
    for when in ("before", "after"):
        assert w[when]["lines_match"] and w[when]["chunks_match"], when
    assert w["before"]["longest"] == [device.MAX_RMST_LINE, device.MAX_RMSN_LINE] == [121, 162]


@pytest.mark.gpu
def test_the_longest_lines_on_the_device(rooms_run):
    part = rooms_run["longest"]
    assert part["n_bad"] == 0, part["first_bad"]
    assert part["rmst"]["bytes"] <= device.MAX_RMST_LINE_BYTES and part["rmsn"]["bytes"] <= device.MAX_RMSN_LINE_BYTES
    assert part["rmst"]["writes"] <= device.MAX_ROOMS_LINE_WRITES and part["rmsn"]["writes"] <= device.MAX_ROOMS_LINE_WRITES
    assert part["rmsn"]["bytes"] > 6 * 100                              # the newlines' room was in it


@pytest.mark.gpu
def test_a_second_run_gives_identical_bytes(rooms_run):
    assert rooms_run["determinism"] == {"same_on_a_second_call": True, "same_on_a_second_roster": True}


@pytest.mark.gpu
def test_nothing_else_moved(rooms_run):
    m = rooms_run["moved"]
    assert m["before_rooms"] == m["fresh"]                              # two rosters built alike: results and copy volumes
    # after rooms_many calls the other calls return what they return on a roster that never saw one; a call may copy less
    # there, never more: a rooms call has uploaded the table, the speaker state or the room table already
    for call, parts in m["fresh_again"].items():
        assert m["after_rooms"][call][:-1] == parts[:-1], call
        assert all(x <= y for x, y in zip(m["after_rooms"][call][-1], parts[-1])), call
    for call in ("look", "who"):
        assert m["listed_after_rooms"][call][:-1] == m["listed_fresh"][call][:-1] and m["listed_after_rooms"][call][-1] <= m["listed_fresh"][call][-1]
    assert m["relay_after_rooms"][:-1] == m["relay_fresh"][:-1] and m["relay_after_rooms"][-1] <= m["relay_fresh"][-1]
    assert m["still_right"]
    h, nr = m["rooms_h2d"], m["look_rooms"]
    # clean mirrors: the lookers alone, a 256-byte slice, and the violation count
    assert len(set(h["clean"] + [h["clean_again"], h["after_updates_of_others"]])) == 1 and h["clean"][0] == 256 + 4
    # the room table is 1,072 bytes per room rounded up to a 256-byte slice, and lies last of the tables: nothing else travels
    assert 1072 * nr <= h["after_set_rooms"] - h["clean"][0] < 1072 * nr + 256
    # the first call follows other calls that uploaded the table and the speaker state: it carries the room table, and the
    # table's two slices once more from the pinned mirror if its layout made the device allocation grow
    slices = -(-4 * m["capacity"] // 256) * 256 + -(-m["capacity"] // 256) * 256
    assert h["first"] - h["after_set_rooms"] in (0, slices)


@pytest.mark.gpu
def test_rooms_many_meets_a_regrown_allocation(rooms_run):
    g = rooms_run["regrown"]
    assert g["passed_the_room_table_alone"] and g["first_alike"] and g["first_right"], g
    # the table travelled again from the pinned mirror, with the room table: more than the room table and the lookers
    assert g["first_h2d"][0] >= 1072 * 1024 + 5 * 65 + 256 + 4
    assert g["second_alike"] and g["second_right"] and g["counted"] == g["model_counted"] > 0, g
