"""``Roster.who_many``: who(user, 0) composed over the roster on the device (nuts_roster_who and nuts_roster_who_shown of
fanout.hip), ``device.Who``, and the two fields it reads beside look()'s (``Roster.update(last_login=, away=)``).

Host tier (unmarked): everything malformed is rejected before the device library loads, and a rejected call changes no
mirror and no dirty flag; the ``_who`` mirror byte for byte; the Python model of ``who()`` (``who`` of
tests/device_who_child.py) reproduces every who of the recorded session tests/golden/reference_only/who.json, through
the CPU restatement's transducer; ``colour_com_count``'s quirks; the rules of the list on hand-built rosters; the longest
line stays within its bounds on the CPU restatement; a ``Who`` built by hand obeys its contract; and over a library that
computes nothing, ``who_many`` is passed exactly the mirrors whose flags were set, also interleaved with the other calls.
In the recorded session every login is seconds old, so ``mins`` is 0 throughout: nonzero and negative ``mins``, and
``away``, are tested against the model only.  The kernels' scratch-free compile is tests/test_device_fanout.py's, which
looks at every function of fanout.hip.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_who_child.py, under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

import child_run
from device_look_child import set_rooms
from device_who_child import (CAPACITIES, DATE, EDGES, LOOKERS_PER_CALL, QUIRK_DESCS, cases, colour_com_count, fuzz_rooms, golden_whos,
                              listed, model_chunks, replay_whos, seat, shown, who, who_line, who_user, worst_user)
from nuts333_amd import device, nuts_path

REPO = Path(__file__).resolve().parent.parent
FLAGS = ("_dirty", "_speech_dirty", "_private_dirty", "_afk_dirty", "_rooms_dirty", "_udesc_dirty", "_who_dirty", "_clones_dirty")


def flags(r):
    return tuple(getattr(r, f) for f in FLAGS)


def clean(r):
    for f in FLAGS:
        setattr(r, f, False)


def seated(capacity=6, **kw) -> device.Roster:
    """A roster over fuzz_rooms() whose slots 0 and 1 stand in room 0; rooms 3, 4 and 5 have a netlink."""
    rooms = fuzz_rooms()
    r = device.Roster(capacity, look_rooms=len(rooms), **kw)
    set_rooms(r, rooms)
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
    assert device.WHO_KERNELS[0] == "nuts_roster_who" and not set(device.WHO_KERNELS) & set(device.KERNELS)
    source = device.SOURCE.read_text()
    for k in device.WHO_KERNELS:
        assert f"{k}(WhoArgs a)" in source
    assert (device.WHO_HEAD_LOGIN, device.WHO_HEAD, device.WHO_FOOT, device.WHO_TAIL) == (0, 1, 2, 3)
    assert device.LEVEL_NAMES == (b"NEW", b"USER", b"WIZ", b"ARCH", b"GOD") and device.WHO_DATE_LEN == 79
    assert (device.MAX_WHO_LINE, device.MAX_WHO_LINE_BYTES, device.MAX_WHO_LINE_WRITES) == (233, 1402, 3)
    assert device.MAX_WHO_LINE <= device._WHO_ROW == 236 < device.TEXT_SIZE


@pytest.mark.parametrize("fields, why", [
    ({"last_login": -1}, "last_login"), ({"last_login": 2**31}, "last_login"), ({"last_login": 1.0}, "last_login"),
    ({"last_login": True}, "last_login"), ({"last_login": None}, "last_login"), ({"last_login": "5"}, "last_login"),
    ({"last_login": [1]}, "1 values for 2 slots"), ({"last_login": [1, -1]}, "last_login"),
    ({"away": 6}, "no room record"), ({"away": -1}, "no room record"), ({"away": True}, "away"), ({"away": "3"}, "away"),
    ({"away": 0}, "room 0 has no netlink"), ({"away": [3, 1]}, "room 1 has no netlink"), ({"away": [3]}, "1 values for 2 slots"),
    ({"last_login": 5, "away": 2}, "room 2 has no netlink"), ({"last_login": 5, "level": 9}, "level"),
    ({"away": 3, "room": -2}, "room"),
])
def test_a_rejected_update_changes_no_mirror(no_library, fields, why):
    r = seated()
    r.update([0, 1], last_login=[7, 8], away=[None, 4])
    clean(r)
    table, speech, whom = r._table.copy(), r._speech.copy(), r._who.copy()
    with pytest.raises(ValueError, match=why):
        r.update([0, 1], **fields)
    assert np.array_equal(r._table, table) and np.array_equal(r._speech, speech) and np.array_equal(r._who, whom)
    assert flags(r) == (False,) * len(FLAGS)


def test_the_who_mirror_byte_for_byte(no_library):
    r = seated(4)
    assert r._who.dtype == np.int32 and r._who.shape == (4, 2) and r._who.nbytes == 4 * device._WHO_REC
    assert r._who.tobytes() == (b"\0\0\0\0" + b"\xff\xff\xff\xff") * 4 and r._who_dirty
    clean(r)
    r.update([1, 3, 1], last_login=[5, 2**31 - 1, 0x01020304])         # the last value of a slot wins
    assert flags(r) == tuple(f == "_who_dirty" for f in FLAGS)
    clean(r)
    r.update(2, away=4)
    assert flags(r) == tuple(f == "_who_dirty" for f in FLAGS)
    r.update([0, 2], away=[5, None])
    assert r._who.tobytes() == (b"\0\0\0\0\5\0\0\0" + b"\4\3\2\1\xff\xff\xff\xff" + b"\0\0\0\0\xff\xff\xff\xff"
                                + b"\xff\xff\xff\x7f\xff\xff\xff\xff")
    clean(r)
    r.update(0, last_login=1, colour=1)                                 # with a field of the table: both
    assert flags(r) == tuple(f in ("_who_dirty", "_dirty") for f in FLAGS)
    clean(r)
    r.update(0, desc=b"x", away=None)
    assert flags(r) == tuple(f in ("_who_dirty", "_udesc_dirty") for f in FLAGS)
    clean(r)
    r.update(0)                                                         # as before: an update of nothing marks the table
    assert flags(r) == tuple(f == "_dirty" for f in FLAGS)


@pytest.mark.parametrize("slots", [[], (), None, 3, "01", b"01"])
def test_slots_must_be_a_non_empty_sequence(no_library, slots):
    with pytest.raises(ValueError, match="slots|empty call"):
        seated().who_many(slots, now=0, date=DATE)


@pytest.mark.parametrize("kw, why", [
    ({"now": -1}, "now"), ({"now": 2**31}, "now"), ({"now": 1.5}, "now"), ({"now": None}, "now"), ({"now": True}, "now"),
    ({"date": b"d" * 80}, "date"), ({"date": b"a\0b"}, "date"), ({"date": 5}, "date"), ({"date": None}, "date"),
    ({"date": "Ā"}, "outside one byte"),
])
def test_now_and_date_are_checked(no_library, kw, why):
    r = seated()
    clean(r)
    with pytest.raises(ValueError, match=why):
        r.who_many([0], **{"now": 0, "date": DATE, **kw})
    assert flags(r) == (False,) * len(FLAGS)


def test_who_many_takes_keywords_only(no_library):
    with pytest.raises(TypeError):
        seated().who_many([0], 0, DATE)


def test_lookers_and_listed_slots_are_checked(no_library):
    r = seated()
    for bad, why in (([0, 6], "who 1: slot"), ([0, 1, -1], "who 2: slot"), ([None], "who 0: slot"), ([True], "who 0: slot")):
        with pytest.raises(ValueError, match=why):
            r.who_many(bad, now=0, date=DATE)
    r.update(2, room=6, name=b"Carol")                                  # room 6 has no record
    clean(r)
    with pytest.raises(ValueError, match="who: slot 2 is in room 6, which has no room record"):
        r.who_many([0], now=0, date=DATE)
    r.update(2, room=None)                                              # roomless, and not away
    clean(r)
    with pytest.raises(ValueError, match="who: slot 2 is in no room and is not away"):
        r.who_many([0], now=0, date=DATE)
    assert flags(r) == (False,) * len(FLAGS)
    r.update(2, away=3)
    r.set_rooms(3, netlink=None)                                        # the link went away after the update
    clean(r)
    with pytest.raises(ValueError, match="who: slot 2 is in no room and is not away"):
        r.who_many([0], now=0, date=DATE)
    assert flags(r) == (False,) * len(FLAGS)
    r.update(2, login=1)                                                # at login stage it is not listed: nothing to check
    with pytest.raises(AssertionError, match="library was loaded"):
        r.who_many([2], now=0, date=DATE)                               # ... and may itself look
    r.close()
    with pytest.raises(ValueError, match="closed"):
        r.who_many([0], now=0, date=DATE)
    with pytest.raises(ValueError, match="closed"):
        r.update(0, last_login=1)


def test_a_call_past_the_cap_is_refused(no_library, monkeypatch):
    r = seated()
    monkeypatch.setattr(device, "MANY_ARENA_CAP", 12 * (304 + 2 * 236) + 16 * 6 + 4 - 1)
    with pytest.raises(ValueError, match="call too large: its variant and bitmap bound is 9412 bytes.*MANY_ARENA_CAP.*split it"):
        r.who_many([0], now=0, date=DATE)


# ------------------------------------------------------------------ host tier: the model
def test_colour_com_count_is_not_the_transducers_count():
    """The eleven values of the issue: the count of a bare command, of the chains, of an escaped and of a cut command,
    and the widest line's."""
    for s, want in ((b"~FR", 1), (b"~FBK", 2), (b"~OLI", 2), (b"~FBBM", 3), (b"~FBBT", 3), (b"~~FR", 1), (b"trailing ~", 0),
                    (b"trailing ~F", 0), (b"  Abcdefghijkl " + b"~FBBM" * 6 + b"~RS", 19)):
        assert colour_com_count(s) == want, s
    line = who_line(worst_user(0), fuzz_rooms(), 0)
    assert line.index(b" : ") == 97 == 40 + 3 * 19                      # the pad width
    assert nuts_path.transduce(b"~FBBM", 1) == b"\x1b[34mBM\x1b[0m"      # one command and two letters to the transducer
    # the bound the kernel and the row rely on: no name and description count more than 25
    assert max(colour_com_count(b"  %s %s~RS" % (n, d)) for n in (b"~FBBM~OLI~FR", b"~FBBM~FBBM~~", b"~OLI~OLI~OLI")
               for d in QUIRK_DESCS) == 25 == device.MAX_WHO_COUNT


def test_the_model_reproduces_the_recorded_session():
    res = replay_whos(lambda users, rooms, slot, now, date: b"".join(model_chunks(users, rooms, slot, now, date)))
    assert res["mismatches"] == [] and res["compared"] == golden_whos() == 9
    assert res["kinds"] == {"colour": 3, "plain": 5, "prompt": 1}
    doc = json.loads((REPO / "tests" / "golden" / "reference_only" / "who.json").read_text())
    text = "".join(s["recv"].get(s["actor"], "") for s in doc["steps"] if s.get("send") in (".who", "who"))
    for needle in ("* Dave", "(AFK)", ": hallway ", ": NEW ", ": ARCH ", ": GOD ", "1 invisible", "\x1b[44m*** Current users DATE"):
        assert needle in text, needle
    assert {a["level"] for a in doc["accounts"][0]} == {0, 1, 2, 3, 4}


def hand_users():
    rooms = fuzz_rooms()
    users = {0: who_user(0, name=b"Zero", room=0, level=2, colour=1, last_login=100),
             1: who_user(1, name=b"Hidden", room=1, level=2, vis=0, desc=b"is a wiz"),
             2: who_user(2, name=b"Below", room=2, level=1, afk=1),
             3: who_user(3, name=b"Above", room=1, level=3, desc=b"~FBKtwo"),
             4: who_user(4, name=None, room=0),                         # no user
             5: who_user(5, name=b"Prompt", room=0, login=1, level=0),  # at login stage, with a room
             6: who_user(6, name=b"Away", room=None, away=4, level=4, last_login=2**31 - 1),
             7: who_user(7, name=None, room=None, login=1, level=0)}    # at the name prompt
    return users, rooms


def test_the_rules_of_the_list():
    users, rooms = hand_users()
    assert listed(users) == [0, 1, 2, 3, 6]
    assert shown(users, 0) == [0, 1, 2, 3, 6] and shown(users, 1) == [0, 1, 2, 3, 6]        # at equal level, and itself
    assert shown(users, 2) == [0, 2, 3, 6] and shown(users, 3) == [0, 1, 2, 3, 6]           # from below, from above
    assert shown(users, 5) == shown(users, 7) == [0, 2, 3, 6]                               # not listed, yet they look
    texts = {j: who(users, rooms, j, 160, DATE) for j in users}
    assert len({tuple(t[-2:]) for t in texts.values()}) == 1                                # the footer: whoever looks
    assert texts[2][-2] == b"\nThere are 4 visible, 1 invisible, 0 remote users.\nTotal of 5 users" and texts[2][-1] == b".\n\n"
    assert texts[0][0] == b"\n~BB*** Current users DATE ***\n\n" and texts[5][0] == texts[7][0] == b"\n*** Current users DATE ***\n\n"
    assert texts[0][1] == b"  Zero ~RS" + b" " * 33 + b" : WIZ  : " + b"R" * 20 + b" : 1 mins.\n"    # 20 bytes in %-12s
    assert texts[0][2] == b"* Hidden is a wiz~RS" + b" " * 23 + b" : WIZ  : twelve_bytes : 2 mins.\n"
    assert texts[0][3] == b"  Below ~RS" + b" " * 32 + b" : USER : e            : 2 mins.~BR(AFK)\n"
    assert texts[0][4].startswith(b"  Above ~FBKtwo~RS" + b" " * 31 + b" : ARCH : ")              # 40 + 3 * 3 wide
    assert texts[0][5] == b"  Away ~RS" + b" " * 33 + b" : GOD  : @" + b"s" * 80 + b" : -35791391 mins.\n"
    assert b"".join(texts[2]).count(b"Hidden") == 0


@pytest.mark.parametrize("last_login, now, mins", [(1061, 1000, b"-1"), (1059, 1000, b"0"), (1060, 1000, b"-1"), (1000, 1059, b"0"),
                                                   (1000, 1060, b"1"), (0, 2**31 - 1, b"35791394"), (2**31 - 1, 0, b"-35791394"),
                                                   (0, 0, b"0")])
def test_mins_truncates_toward_zero(last_login, now, mins):
    line = who_line(who_user(0, name=b"A", last_login=last_login), fuzz_rooms(), now)
    assert line.endswith(b" : " + mins + b" mins.\n")


def test_an_empty_talker():
    users = {0: who_user(0, name=None, room=None, login=1)}
    assert who(users, fuzz_rooms(), 0, 5, b"") == [b"\n*** Current users  ***\n\n",
                                                   b"\nThere are 0 visible, 0 invisible, 0 remote users.\nTotal of 0 users", b".\n\n"]


def test_the_longest_line_stays_within_its_bounds():
    """A 12-byte name, the 19-count description, ``@`` and an 80-byte service, the widest mins, AFK: 215 bytes; and with a
    name that counts too, 233, the row's reason.  MAX_WHO_LINE_BYTES is the transducer's own bound for that length."""
    rooms = fuzz_rooms()
    assert device.MAX_WHO_LINE_BYTES == device.max_bytes(device.MAX_WHO_LINE)
    longest = 0
    for u in (worst_user(0), worst_user(0, vis=0), worst_user(0, name=b"~FBBM~OLI~FR"), worst_user(0, name=b"\n" * 12, desc=b"\n" * 30),
              worst_user(0, desc=b"~FR" * 10), worst_user(0, last_login=0)):
        for now in (0, 2**31 - 1):
            line = who_line(u, rooms, now)
            longest = max(longest, len(line))
            for c in (0, 1):
                ch = nuts_path.chunks(line, c)
                assert sum(map(len, ch)) <= device.MAX_WHO_LINE_BYTES and len(ch) <= device.MAX_WHO_LINE_WRITES
    assert len(who_line(worst_user(0), rooms, 0)) == 215 and longest == device.MAX_WHO_LINE == 233
    head = b"\n~BB*** Current users %s ***\n\n" % (b"d" * device.WHO_DATE_LEN)
    foot = b"\nThere are %d visible, %d invisible, %d remote users.\nTotal of %d users" % (65536, 65536, 0, 65536)
    gaps = [b - a for a, b in zip(device._WHO_FIXED_AT, device._WHO_FIXED_AT[1:] + (device._WHO_FIXED_STRIDE,))]
    assert [len(head) - 3, len(head), len(foot), 3] == [104, 107, 79, 3] and all(n <= g for n, g in zip([104, 107, 79, 3], gaps))


# ------------------------------------------------------------------ the dataclass
def hand_built_who():
    """A Who from the model alone: texts and variants scattered over buffers of 0xAA bytes, -7 in the unused chunk sizes."""
    users, rooms = hand_users()
    for j in range(8, 42):                                              # 39 listed users: two bitmap words
        users[j] = who_user(j, name=b"U%d" % j, room=j % 3, level=j % 5, vis=int(j % 4 != 0))
    slots, order = [0, 2, 7, 0, 41], listed(users)
    strings = {0: b"\n*** Current users DATE ***\n\n", 1: b"\n~BB*** Current users DATE ***\n\n"}
    strings[2], strings[3] = who(users, rooms, 0, 160, DATE)[-2:]
    strings.update({4 + l: who_line(users[j], rooms, 160) for l, j in enumerate(order)})
    T = len(strings)
    texts, variants = np.full(8000, 0xAA, dtype=np.uint8), np.full(40_000, 0xAA, dtype=np.uint8)
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
    bits = np.zeros((len(slots), 2), dtype=np.uint32)
    for k, s in enumerate(slots):
        for l, j in enumerate(order):
            if j in shown(users, s):
                bits[k, l // 32] |= np.uint32(1 << (l % 32))
    w = device.Who(slots=np.array(slots, dtype=np.int32), colour=np.array([users[s]["colour"] for s in slots], dtype=np.uint8),
                   login=np.array([users[s]["login"] for s in slots], dtype=np.uint8), line_slots=np.array(order, dtype=np.int32),
                   shown=bits, texts=texts, text_starts=tstarts, text_sizes=tsizes, variants=variants, variant_starts=starts,
                   variant_sizes=sizes, write_counts=counts, write_sizes=wsz)
    return w, users, rooms, slots


def test_a_hand_built_who_obeys_the_contract(no_library):
    w, users, rooms, slots = hand_built_who()
    order = listed(users)
    assert w.timing == {} and len(order) == 39 and w.shown.shape == (5, 2)
    for k, slot in enumerate(slots):
        assert w.chunks(k) == model_chunks(users, rooms, slot, 160, DATE) and w.output(k) == b"".join(w.chunks(k))
        assert [order[l] for l in w.lines(k)] == shown(users, slot)
        assert [w.text(t) for t in w.text_numbers(k)] == who(users, rooms, slot, 160, DATE)
    assert w.text_numbers(2)[0] == device.WHO_HEAD_LOGIN and w.text_numbers(0)[0] == device.WHO_HEAD
    assert w.text_numbers(0)[-2:] == [device.WHO_FOOT, device.WHO_TAIL]
    assert w.chunks(0) == w.chunks(3) and w.chunks(0)[-1] == b"\x1b[0m"             # the same looker twice; colour on
    assert len(w.lines(1)) < len(w.lines(0)) and b"\x1b" not in w.output(1)
    w.shown[:, 1] |= np.uint32(0xFFFFFF80)                                          # bits at or past L are nobody's lines
    assert [order[l] for l in w.lines(0)] == shown(users, 0)
    for bad_k in (-1, 5):
        for call in (w.chunks, w.output, w.lines, w.text_numbers):
            with pytest.raises(IndexError):
                call(bad_k)
    for bad_t in (-1, 4 + 39):
        with pytest.raises(IndexError):
            w.text(bad_t)
        with pytest.raises(IndexError):
            w.text_chunks(bad_t, 0)
    with pytest.raises(IndexError):
        w.text_chunks(0, 2)


# ------------------------------------------------------------------ dirty flags, over a library that computes nothing
MIRRORS = ("_table", "_speech", "_rooms", "_udesc", "_who", "_afk", "_clones")
WHO_MIRROR_ARGS = dict(zip(range(7, 12), ("_table", "_speech", "_rooms", "_udesc", "_who")))


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


def test_who_many_is_passed_exactly_the_dirty_mirrors(fake):
    r = seated(8, clones=2, review_rooms=2)
    w = r.who_many([0, 1, 0], now=9, date=b"on a day")
    name, args = fake.calls[-1]
    assert name == "nd_roster_who" and args[1] == 3 and args[3] == 2 and args[4] == 9 and args[6] == 8
    assert [m for i, m in WHO_MIRROR_ARGS.items() if args[i] is not None] == ["_table", "_speech", "_rooms", "_udesc", "_who"]
    assert all(args[i] == getattr(r, m).ctypes.data for i, m in WHO_MIRROR_ARGS.items())
    assert flags(r) == tuple(f in ("_afk_dirty", "_clones_dirty") for f in FLAGS)           # not who_many's to clear
    assert w.shown.shape == (3, 1) and w.shown.dtype == np.uint32 and len(w.text_sizes) == 6 and w.login.tolist() == [0, 0, 0]
    r.who_many([0], now=9, date=DATE)
    assert passed(fake, r) == set()
    for fields, mirrors in (({"last_login": 3}, {"_who"}), ({"away": 3}, {"_who"}), ({"desc": b"d"}, {"_udesc"}), ({"afk": 1}, {"_speech"}),
                            ({"level": 3}, {"_speech"}), ({"vis": 0}, {"_speech"}), ({"login": 1}, {"_table"}), ({"room": 1}, {"_table"}),
                            ({"igntell": 1}, {"_speech"}), ({"afk_mesg": b"brb"}, set()), ({"last_login": 4, "name": b"Zed"}, {"_who", "_speech"})):
        r.update(1, **fields)
        r.who_many([0], now=9, date=DATE)
        assert passed(fake, r) == mirrors, fields
        r.who_many([0], now=9, date=DATE)
        assert passed(fake, r) == set(), fields
    r.set_rooms(2, name=b"renamed")
    r.who_many([0], now=9, date=DATE)
    assert passed(fake, r) == {"_rooms"} and not r._rooms_dirty
    r.set_clones(0, owner=0, room=0, hear=2)
    r.who_many([0], now=9, date=DATE)
    assert passed(fake, r) == set() and r._clones_dirty and r._afk_dirty


def test_who_many_interleaved_with_the_other_calls(fake):
    """No call reads a stale field, and no existing call is passed more than on a roster that never saw a who."""
    def build():
        r = seated(8, clones=2, review_rooms=2, revtell=True)
        r.set_clones(0, owner=0, room=0, hear=2)
        return r

    calls = {"look": lambda r: r.look_many([0, 1]), "relay": lambda r: r.relay_many([(b"hi\n", 0, 1, 0, 3)]),
             "tell": lambda r: r.tell_many([(0, device.COM_TELL, b"bobby psst", 3)]),
             "speak": lambda r: r.speak_many([(0, device.COM_SAY, b"hello", 1)]),
             "who": lambda r: r.who_many([0, 1], now=5, date=DATE)}
    reads = {"look": {"_table", "_speech", "_rooms", "_udesc"}, "relay": {"_table", "_clones"}, "tell": {"_table", "_speech", "_afk"},
             "speak": {"_table", "_speech"}, "who": {"_table", "_speech", "_rooms", "_udesc", "_who"}}
    updates = (({"last_login": 9}, {"_who"}), ({"away": 4}, {"_who"}), ({"desc": b"new"}, {"_udesc"}), ({"vis": 0}, {"_speech"}),
               ({"level": 2}, {"_speech"}), ({"room": 1}, {"_table"}), ({"colour": 1}, {"_table"}), ({"afk_mesg": b"brb"}, {"_afk"}))
    order = ["who", "look", "who", "relay", "tell", "who", "speak", "look", "who", "tell", "relay", "speak"]
    with_who, without = build(), build()
    for r in (with_who, without):
        stale, handed = set(MIRRORS), {}
        for n, (fields, mirrors) in enumerate(updates * 3):
            r.update(n % 2, **fields)
            stale |= mirrors
            for kind in [k for k in order[n % 4:] + order[:n % 4] if r is with_who or k != "who"]:
                calls[kind](r)
                got = passed(fake, r)
                assert got <= stale and not (reads[kind] - got) & stale, (n, kind, got, stale)
                stale -= got
                if kind != "who":
                    handed[kind] = handed.get(kind, 0) + sum(getattr(r, m).nbytes for m in got)
        r.volume = handed
    assert all(with_who.volume[k] <= without.volume[k] for k in without.volume)
    # the room table is one mirror for look_many and who_many: whoever uploads it clears the flag for both
    r = build()
    r.who_many([0], now=1, date=DATE)
    r.look_many([0])
    assert "_rooms" not in passed(fake, r)
    r.set_rooms(0, topic=b"t")
    r.look_many([0])
    r.who_many([0], now=1, date=DATE)
    assert "_rooms" not in passed(fake, r)
    r.relay_many([(b"hi\n", 0, 1, 0, 3)])                               # relay_many's own path for the names is untouched
    assert fake.calls[-1][0] == "nd_roster_relay"


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def who_run(built):
    res = child_run.run_child("device_who_child.py", "DEVICE_WHO", 300)
    print("\n[who]", json.dumps(res)[:4000])
    return res


@pytest.mark.gpu
def test_the_recorded_session_replays_on_the_device(who_run):
    g = who_run["golden"]
    assert g["compared"] == golden_whos() == 9 and g["kinds"] == {"colour": 3, "plain": 5, "prompt": 1}
    assert g["mismatches"] == [] and g["n_bad_vs_model"] == 0, g


@pytest.mark.gpu
def test_seeded_whos_match_the_model(who_run):
    f = who_run["fuzz"]
    assert f["capacities"] == list(CAPACITIES) == [1, 64, 65, 257, 1025] and LOOKERS_PER_CALL == 8
    assert f["calls"] == len(cases()) and f["listed"] == sorted(set(EDGES) | {1025}) == [0, 1, 31, 32, 33, 63, 64, 65, 256, 257, 1025]
    assert f["levels"] == [0, 1, 2, 3, 4] and f["colours"] == [0, 1] and f["login_lookers"] > 0
    assert f["hidden_by_level"] > 0 and f["afk"] > 0 and f["away"] > 0 and f["negative_mins"] > 0
    assert {1, 2, 3, 4, 19} <= set(f["quirk_counts"]) and max(f["quirk_counts"]) <= device.MAX_WHO_COUNT
    assert f["dense"] >= 4 and f["sparse"] >= 4
    assert f["n_bad"] == 0, f["first_bad"]


@pytest.mark.gpu
def test_the_longest_line_on_the_device(who_run):
    for now, part in who_run["worst"].items():
        assert part["n_bad"] == 0, (now, part["first_bad"])
        assert part["most_bytes"] <= device.MAX_WHO_LINE_BYTES and part["most_writes"] <= device.MAX_WHO_LINE_WRITES
    assert who_run["worst"]["0"]["longest"] == device.MAX_WHO_LINE == 233


@pytest.mark.gpu
def test_a_second_run_gives_identical_bytes(who_run):
    assert who_run["determinism"] == {"same_on_a_second_call": True, "same_on_a_second_roster": True}


@pytest.mark.gpu
def test_nothing_else_moved(who_run):
    m = who_run["moved"]
    assert m["before_who"] == m["fresh"]                                # two rosters built alike: results and copy volumes
    # after who_many calls the other calls return what they return on a roster that never saw one; a call may copy less
    # there, never more: a who call that found the allocation grown has uploaded the table again already
    for call, parts in m["fresh_again"].items():
        assert m["after_who"][call][:-1] == parts[:-1], call
        assert all(x <= y for x, y in zip(m["after_who"][call][-1], parts[-1])), call
    assert m["look_after_who"][0] == m["look_fresh"][0] and m["look_after_who"][1] <= m["look_fresh"][1]
    h, cap = m["who_h2d"], m["capacity"]
    # clean mirrors: the lookers and the date alone, a 256-byte slice each, and the violation count
    assert len(set(h["clean"] + [h["clean_again"]])) == 1 and h["clean"][0] == 2 * 256 + 4
    # the who table is 8 bytes per slot rounded up to a 256-byte slice, and lies last: nothing else travels with it
    assert 8 * cap <= h["after_last_login_update"] - h["clean"][0] < 8 * cap + 256
    # the descriptions lie in front of it, so it travels with them: two slices
    assert 40 * cap <= h["after_desc_update"] - h["clean"][0] < 40 * cap + 512
    assert h["first"] > h["after_desc_update"]                          # the table, the speaker state and the rooms as well
