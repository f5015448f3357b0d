"""The device work of tests/test_device_limits.py, in a short-lived child process of its own, and the roster descriptions
and scripts its host tier shares with it.

As the other device children: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_LIMITS {...}``).  Every call of a ``device.Roster`` runs here at the sizes the API accepts and no
other device test reaches: 65,536 slots, 1,024 look rooms, 1,024 review rooms, 65,536 clone records, revtell rings.

* ``edge``: one sparse roster at every limit at once, users at the first and last slots of the first, second, middle
  and last tiles, rooms 0, 1, 511, 1022 and 1023, clone records up to 65,535.  Every call once or twice, every byte,
  chunk size, bitmap word and list against the models; then slot 65,535, record 65,535 and room 1,023 are updated alone
  and one call of each table-reading kind is repeated.
* ``full``: every slot a named user.  who, look, tell, plan and broadcast where the counts themselves are the edge.
* ``guards``: a plan of 4,096 broadcasts to 65,536 slots, 2^28 admit bits, against the numpy predicate word by word.

The expected values are the models the other children hold to the recorded sessions: ``who`` / ``who_line``
(device_who_child), ``look`` (device_look_child), ``private`` (device_tell_child), ``relays`` (device_relay_child),
``model`` (device_speak_child), ``answer_of`` (device_input_child), ``Rings`` (device_review_child), ``TellRings``, and
``nuts_path.chunks`` for every transduced text.  The one statement of its own is ``admits_np``, ``np_fanout_admits`` over
arrays, which the host tier holds to ``nuts_path.admits`` over the full truth table: a bitmap of 65,536 slots cannot be
compared cell by cell through ctypes.

    python tests/device_limits_child.py
"""
from __future__ import annotations

import ctypes
import json
import random
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from device_input_child import answer_of, input_differences, new_counts as input_counts  # noqa: E402
from device_look_child import look_differences, members, new_counts as look_counts, new_room  # noqa: E402
from device_relay_child import ALL, NOTHING as HEAR_NOTHING, SWEARS, new_counts as relay_counts, relay_differences, relays  # noqa: E402
from device_review_child import Rings, review_differences  # noqa: E402
from device_speak_child import EMOTE, SAY, SEMOTE, SHOUT, model as speech_model, speech_differences  # noqa: E402
from device_tell_child import PEMOTE, TELL, TellRings, new_counts as tell_counts, private, private_differences  # noqa: E402
from device_who_child import (colour_com_count, listed, new_counts as who_counts, shown, who, who_differences, who_line,  # noqa: E402
                              who_user)
from nuts333_amd import device, nuts_path  # noqa: E402

CAPACITY = device.MAX_CAPACITY
EDGE_SLOTS = (0, 255, 256, 257, 32767, 32768, 65279, 65280, 65534, 65535)
EDGE_ROOMS = (0, 1, 511, 1022, 1023)
EDGE_CLONES = (0, 63, 64, 255, 256, 32768, 65535)
LAST = CAPACITY - 1
LAST_ROOM = device.MAX_LOOK_ROOMS - 1
RANDOM_SLOTS = 50
NOW, DATE = 1_800_000_000, b"on Monday 19 October 2026 at 12:29"
#: what a user of these rosters carries: every field some model reads
FIELDS = ("room", "login", "ignall", "ignshout", "colour", "name", "vis", "muzzled", "command_mode", "level", "afk", "igntell",
          "afk_mesg", "desc", "last_login", "away")
DESCS = (b"~FBBM" * 6, b"is a user", b"", b"~FR/", b"ends in ~F", b"~ULI~RVS", b"\xe9\xff high", b"x" * 30, b"~FBK two", b"~~FR")
#: the plan of part 3: 4,096 broadcasts to 65,536 slots are 2^28 admit bits
GUARD_K = 4096
GUARD_LINES = (b"one\n", b"~FRtwo~RS\n", b"three /~FG escaped\n", b"", b"~OLfive shouts:~RS loud\n", b"six\n\n", b"seven ~", b"8",
               b"\xe9ine\n", b"ten " * 10 + b"\n")


# ------------------------------------------------------------------ the admit predicate over arrays
def admits_np(login, has_room, same_room, ignall, ignshout, is_sender, rm_is_null, force_listen, com_num):
    """np_fanout_admits (oracle/nuts_path.c) over boolean arrays of any shapes that broadcast, ``com_num`` an int array."""
    shout = (com_num == device.COM_SHOUT) | (com_num == device.COM_SEMOTE)
    return (~login & has_room & (same_room | rm_is_null) & (~ignall | force_listen) & ~(ignshout & shout) & ~is_sender)


def broadcast_arrays(bs):
    """The rooms (-1: every room), senders (-1: none), force_listen flags and commands of ``(text, rm, sender, force_listen,
    com_num)`` tuples."""
    return (np.array([-1 if b[1] is None else b[1] for b in bs], dtype=np.int64),
            np.array([-1 if b[2] is None else b[2] for b in bs], dtype=np.int64),
            np.array([bool(b[3]) for b in bs]), np.array([b[4] for b in bs], dtype=np.int64))


def admit_words(room: np.ndarray, flags: np.ndarray, bs, step: int = 64) -> np.ndarray:
    """uint64 [K, ceil(capacity / 64)]: the admit bitmap of every broadcast over a roster's ``room`` and ``flags`` mirrors, the
    listener fields derived as ``Roster.table`` derives them; ``step`` broadcasts at a time, never K x capacity booleans."""
    cap, k = len(room), len(bs)
    words = (cap + 63) // 64
    rms, senders, fls, coms = broadcast_arrays(bs)
    bit = device.ROSTER_FLAGS
    login, ignall, ignshout = ((flags & bit[f]) != 0 for f in ("login", "ignall", "ignshout"))
    slots = np.arange(cap)
    out = np.zeros((k, words), dtype=np.uint64)
    for lo in range(0, k, step):
        rm, sender = rms[lo:lo + step, None], senders[lo:lo + step, None]
        ok = np.zeros((len(rm), 64 * words), dtype=bool)
        ok[:, :cap] = admits_np(login[None], (room >= 0)[None], (room[None] == rm) & (rm >= 0), ignall[None], ignshout[None],
                                slots[None] == sender, rm < 0, fls[lo:lo + step, None], coms[lo:lo + step, None])
        out[lo:lo + step] = np.packbits(ok, axis=1, bitorder="little").view("<u8")
    return out


# ------------------------------------------------------------------ the rosters, described
def user(slot: int, **fields) -> dict:
    return who_user(slot, **{"ignshout": 0, "room": 0, "last_login": NOW - 60 * (slot % 1000), **fields})


def edge_description(seed: int = 20262):
    """The sparse roster of part 1: ``users`` by slot, ``rooms`` by room, ``records`` for all 65,536 clone records (owner
    None: empty).  Pure: the host tier reads the same description."""
    rng = random.Random(seed)
    rooms = {
        0: new_room(b"first", links=[1, LAST_ROOM], topic=b"the first room", netlink=(b"alpha", False), desc=b"Room zero.\n", mesg_cnt=7),
        1: new_room(b"second_room_", access=device.PRIVATE, links=[0, 511], topic=b"~FRred topic", netlink=(b"beta", True)),
        511: new_room(b"M" * 20, access=device.FIXED_PUBLIC, links=[1, 1022, 0], topic=b"t", netlink=(b"s" * 80, False),
                      desc=b"d" * device.ROOM_DESC_LEN),
        1022: new_room(b"~FRred/", access=device.FIXED_PRIVATE, links=list(EDGE_ROOMS), topic=b"x" * device.TOPIC_LEN,
                       netlink=(b"gamma", True), mesg_cnt=2**31 - 1),
        LAST_ROOM: new_room(b"last_room", links=[1022, 0], topic=b"the last room's topic", netlink=(b"omega-link", False),
                            desc=b"The last room record of the table.\n~FGgreen~RS\n", mesg_cnt=1023)}
    users = {
        0: user(0, name=b"Zero", room=0, level=0, desc=b"~FBBM" * 6),
        255: user(255, name=b"Tileend", room=0, level=2, colour=1, vis=0, desc=b"is unseen"),
        256: user(256, name=b"Afker", room=LAST_ROOM, level=1, afk=1, afk_mesg=b"gone to the last room", desc=b"~FR/"),
        257: user(257, name=b"Deafy", room=LAST_ROOM, level=3, igntell=1, muzzled=1, colour=1),
        32767: user(32767, name=b"Roamer", room=None, away=LAST_ROOM, level=2, desc=b"is away"),
        32768: user(32768, name=b"Halfway", room=1, ignshout=1, colour=1, level=1),
        65279: user(65279, name=b"Hermit", room=511, ignall=1, level=3, desc=b"ends in ~F"),
        65280: user(65280, name=b"Porter", room=1022, login=1, level=0, colour=1),
        65534: user(65534, name=b"Penult65534", room=LAST_ROOM, level=4, colour=1, command_mode=1, desc=b"~ULI~RVS", last_login=0),
        LAST: user(LAST, name=b"Last", room=LAST_ROOM, level=2, desc=b"holds the last words", last_login=NOW + 61)}
    pool = [j for j in range(CAPACITY) if j not in EDGE_SLOTS]
    for j in sorted(rng.sample(pool, RANDOM_SLOTS)):
        away = rng.random() < 0.1
        users[j] = user(j, name=b"R%d" % j, room=None if away else rng.choice(EDGE_ROOMS), away=LAST_ROOM if away else None,
                        login=int(rng.random() < 0.1), ignall=int(rng.random() < 0.2), ignshout=int(rng.random() < 0.3),
                        colour=rng.randrange(2), vis=int(rng.random() < 0.7), level=rng.randrange(5), afk=int(rng.random() < 0.2),
                        igntell=int(rng.random() < 0.2), desc=rng.choice(DESCS), last_login=rng.choice((0, NOW, NOW - 3599, NOW + 600)))
    records = [[None, None, HEAR_NOTHING] for _ in range(CAPACITY)]
    records[0] = [255, 0, ALL]
    records[63] = [65279, LAST_ROOM, ALL]                  # its owner ignores everyone: it never relays
    records[64] = [65534, 0, HEAR_NOTHING]
    records[255] = [256, 511, SWEARS]
    records[256] = [LAST, 1, ALL]
    records[32768] = [LAST, LAST_ROOM, SWEARS]
    records[LAST] = [0, LAST_ROOM, ALL]
    return users, rooms, records


def full_description():
    """The dense roster of part 2: every slot a named user over two rooms; about 1 in 6 invisible, so that the footer's
    invisible count has five digits too, and 1 in 50 at login."""
    users = {}
    for j in range(CAPACITY):
        users[j] = user(j, name=b"U%d" % j, room=int(j % 3 == 0), level=j % 5, vis=int(j % 6 != 3), login=int(j % 50 == 17),
                        colour=j >> 1 & 1, afk=int(j % 11 == 0), ignall=int(j % 13 == 0), ignshout=int(j % 5 == 1),
                        igntell=int(j % 17 == 0), desc=DESCS[j % len(DESCS)], last_login=NOW - 60 * (j % 5000))
    plain = dict(login=0, afk=0, ignall=0, igntell=0, muzzled=0, vis=1)
    users[LAST].update(name=b"Qzedy", **plain)             # an exact name in the last block ...
    users[3].update(name=b"aQzedyb", **plain)              # ... and substring hits in the first and a middle one
    users[40000].update(name=b"Qzedyzz", **plain)
    users[256].update(name=b"U256Mark", **plain)           # a substring in the second tile and in the last
    users[65280].update(name=b"U65280Mark", **plain)
    users[65534].update(name=b"Afker", **{**plain, "afk": 1}, afk_mesg=b"away from the last tile")
    users[65533].update(name=b"Deafy", **{**plain, "igntell": 1}, level=4)
    users[1].update(**plain, level=1)                      # the speakers: below WIZ, and a GOD
    users[4].update(**plain, level=4)
    rooms = {0: new_room(b"hall", links=[1], topic=b"most are here"), 1: new_room(b"annexe", links=[0], access=device.PRIVATE)}
    return users, rooms


#: the lookers of part 2: the lowest and the highest level, and one at login
FULL_WHO_LOOKERS = (5, 4, 17)
#: one looker in each room, the lowest and the highest level
FULL_LOOKERS = (5, 9)
TELL_SPEAKER, TELL_GOD = 1, 4


def full_tell_cases():
    """(name of the case, event, expected outcome, expected target) of part 2's first tell call, and of the one after
    slots 3 and 40000 have been renamed."""
    first = [("exact_in_the_last_block_beats_substrings", (TELL_SPEAKER, TELL, b"qzedy exact beats the substrings", 5), device.TOLD, LAST),
             ("lowest_substring_wins", (TELL_SPEAKER, PEMOTE, b"Mark the lowest slot wins", 5), device.TOLD, 256),
             ("nobody", (TELL_SPEAKER, TELL, b"nobodyatall are you there", 5), device.NOBODY, None),
             ("exact_target_is_afk", (TELL_SPEAKER, TELL, b"afker hello there", 4), device.AFK, 65534),
             ("exact_target_ignores_tells", (TELL_SPEAKER, TELL, b"deafy hello?", 3), device.IGNTELL, 65533),
             ("a_god_is_heard_all_the_same", (TELL_GOD, TELL, b"deafy hello?", 3), device.TOLD, 65533)]
    second = [("substring_of_the_last_name_alone", (TELL_SPEAKER, TELL, b"Qzed only the last slot", 6), device.TOLD, LAST)]
    return first, second


def full_renames():
    return [3, 40000], [b"U3", b"U40000"]


def seat_all(roster: device.Roster, users: dict, rooms: dict) -> None:
    """The whole description in one ``set_rooms`` and one ``update``."""
    ids = sorted(rooms)
    roster.set_rooms(ids, **{f: [rooms[i][f] for i in ids] for f in ("name", "access", "desc", "links", "topic", "mesg_cnt", "netlink")})
    slots = sorted(users)
    roster.update(slots, **{f: [users[j][f] for j in slots] for f in FIELDS})


def seat_clones(roster: device.Roster, records) -> None:
    owned = [c for c, r in enumerate(records) if r[0] is not None]
    roster.set_clones(owned, owner=[records[c][0] for c in owned], room=[records[c][1] for c in owned],
                      hear=[records[c][2] for c in owned])


class SparseTellRings(TellRings):
    """TellRings whose rings come into being when first touched: 65,536 slots, a handful of them told anything."""

    def __init__(self):
        self.ring, self.revline = _Lazy(lambda: ctypes.create_string_buffer(self.LINES * self.SLOT)), _Lazy(lambda: ctypes.c_int(0))


class _Lazy(dict):
    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, key):
        self[key] = self.make()
        return self[key]


# ------------------------------------------------------------------ part 1's script, and what the models make of it
def edge_script() -> dict:
    long_line = b"~FRa long line~RS " + b"\n" * 300 + b"/~FG its end\n"
    s = {}
    s["plan"] = [(b"Last says: ~FRhello~RS to room /~FG 1023\n", LAST_ROOM, LAST, 0, SAY),
                 (b"~OLLast shouts:~RS to every room\n", None, LAST, 0, SHOUT),
                 (b"forced past ignall\n", 511, None, 1, SAY), (b"", 0, 0, 0, SAY), (b"~OL!!~RS Someone semotes\n", None, None, 0, SEMOTE),
                 (long_line, LAST_ROOM, 256, 0, EMOTE), (b"x" * 250 + b"\n", 1, 32768, 1, SAY)]
    s["plan_record"] = [True, False, False, False, False, True, False]
    s["speak"] = [(LAST, SAY, b"hello from the last slot", 5), (0, SAY, b"am I first?", 3), (255, EMOTE, b";waves unseen", 2),
                  (256, SHOUT, b"loud ~FRred~RS words", 3), (65534, SEMOTE, b"#grins at every room", 4), (257, SAY, b"muzzled", 1),
                  (65279, EMOTE, b"nods", 1), (32768, SAY, b"what the shit", 3), (LAST, EMOTE, b";'s line is the ring's last", 6),
                  (LAST, SAY, b"y" * 260, 1), (65534, SAY, b"", 1)]
    s["reads"] = [(LAST, b"hello there from a read\n"), (LAST, b".shout everyone hear this\r\n"), (0, b";smiles\n"), (255, b".\n"),
                  (256, b"\n"), (65534, b"tell zero hi there\n"), (65534, b"say in command mode\n"), (257, b"\xff\xfb\x01"),
                  (32768, b".nosuchcommand\n"), (65279, b"#grins widely\n"), (LAST, b"last read into ring 1023\n"), (0, b".go second\n")]
    s["tell"] = [(LAST, TELL, b"zero hello from the end", 5), (0, TELL, b"last and back again?", 5), (255, PEMOTE, b"last waves", 3),
                 (65534, TELL, b"afker are you there", 5), (0, TELL, b"deafy hi there", 4), (65534, TELL, b"deafy hi from a god", 6),
                 (LAST, TELL, b"roamer come back", 4), (LAST, TELL, b"hermit hello", 3), (LAST, TELL, b"last hi me", 4),
                 (0, TELL, b"nobodyhere hi", 3), (LAST, PEMOTE, b"last grins", 3), (0, TELL, b"65534 by a substring", 5),
                 (0, TELL, b"porter is at login", 5), (257, TELL, b"zero muzzled", 3), (LAST, TELL, b"zero", 2),
                 (65534, PEMOTE, b"Last " + b"z" * 250, 3)]
    s["revtell"] = [LAST, 0, 257, LAST]
    s["review"] = [LAST_ROOM, 0, LAST_ROOM]
    s["look"] = [0, 255, LAST, 256, 65534, 0]
    s["who"] = [0, LAST, 65280]
    s["relay"] = [(b"to the last room\n", LAST_ROOM, LAST, 0, SAY), (b"shit happens in the last room\n", LAST_ROOM, None, 0, SAY),
                  (b"the clone itself speaks\n", LAST_ROOM, None, 0, SAY), (b"room zero\n", 0, 0, 0, SAY),
                  (b"everyone\n", None, LAST, 0, SHOUT), (b"five eleven, shit\n", 511, None, 1, SAY), (b"one\n", 1, None, 0, SAY),
                  (b"L" * (device.ARR_SIZE - 1 - device.RELAY_EXTRA - len(b"last_room") - 1) + b"\n", LAST_ROOM, 0, 0, SAY)]
    s["relay_record"] = [True] + [False] * 7
    s["relay_clone_sender"] = [None, None, LAST, None, None, None, None, None]
    # after the update of slot 65,535, record 65,535 and room 1,023 alone
    s["again_plan"] = [(b"after the update\n", LAST_ROOM, None, 0, SAY), (b"~FRshout~RS after the update\n", None, 0, 0, SHOUT)]
    s["again_speak"] = [(LAST, SAY, b"renamed and still here?", 4), (LAST, SHOUT, b"ignshout is mine now", 4)]
    s["again_reads"] = [(LAST, b".shout a god may\n"), (LAST, b"said after the update\n")]
    s["again_tell"] = [(0, TELL, b"omega found by the new name", 6), (0, TELL, b"last is nobody now", 5), (LAST, TELL, b"deafy a god is heard", 6)]
    s["again_relay"] = [(b"only swearing passes now\n", LAST_ROOM, None, 0, SAY), (b"shit passes\n", LAST_ROOM, None, 0, SAY)]
    return s


def edge_update(users: dict, rooms: dict, records) -> None:
    """What changes after part 1's first round, in the models: slot 65,535, record 65,535 and room 1,023 alone."""
    users[LAST].update(name=b"Omega", colour=1, level=4, desc=b"~FBBM~FBBMnew", last_login=NOW - 120, afk_mesg=b"new", ignshout=1)
    records[LAST][2] = SWEARS
    rooms[LAST_ROOM].update(topic=b"a new topic for the last room", name=b"last_room_renamed")


def apply_edge_update(roster: device.Roster, users: dict, rooms: dict, records) -> None:
    u, rm = users[LAST], rooms[LAST_ROOM]
    roster.update(LAST, **{f: u[f] for f in ("name", "colour", "level", "desc", "last_login", "afk_mesg", "ignshout")})
    roster.set_clones(LAST, hear=records[LAST][2])
    roster.set_rooms(LAST_ROOM, topic=rm["topic"], name=rm["name"])


def record_plan(rings: Rings, bs, record) -> None:
    for (text, rm, *_), on in zip(bs, record):
        if on:
            rings.record(rm, text)


def record_speech(rings: Rings, users: dict, events, ban: bool) -> None:
    for slot, com, inpstr, wc in events:
        m = speech_model(users[slot], com, inpstr, wc, ban)
        if m["recorded"]:
            rings.record(m["rm"], m["line"])


def record_reads(rings: Rings, users: dict, reads, ban: bool) -> None:
    for slot, data in reads:
        _, m = answer_of(users[slot], data, ban)
        if m["recorded"]:
            rings.record(m["rm"], m["line"])


def record_tells(rings: TellRings, users: dict, events) -> None:
    for slot, com, inpstr, wc in events:
        m = private(users, slot, com, inpstr, wc)
        if m["line"] is not None:
            rings.record(m["target"], m["line"])


def edge_coverage() -> dict:
    """What the models alone say part 1 reaches: the planted inputs are the edges they were planted for."""
    users, rooms, records = edge_description()
    s = edge_script()
    rings, trings = Rings(device.MAX_REVIEW_ROOMS), SparseTellRings()
    record_plan(rings, s["plan"], s["plan_record"])
    record_speech(rings, users, s["speak"], True)
    record_reads(rings, users, s["reads"], False)
    record_tells(trings, users, s["tell"])
    ignall = {j: u["ignall"] for j, u in users.items()}
    tells = [private(users, *ev) for ev in s["tell"]]
    return {"slots": sorted(users), "rooms": sorted(rooms), "records": [c for c, r in enumerate(records) if r[0] is not None],
            "hear": sorted({r[2] for r in records if r[0] is not None}),
            "ignall_owner": any(users[r[0]]["ignall"] for r in records if r[0] is not None),
            "roomless_away": [j for j, u in users.items() if u["room"] is None and u["away"] == LAST_ROOM],
            "ring_last_room": len(rings.lines(LAST_ROOM)), "revtell_last": len(trings.lines(LAST)),
            "relays_at_last_record": sum(LAST in relays(records, ignall, b[1], cs, b[0])
                                         for b, cs in zip(s["relay"], s["relay_clone_sender"])),
            "clone_sender_last": s["relay_clone_sender"].count(LAST),
            "most_colour_coms": max(colour_com_count(b"  %s %s~RS" % (u["name"], u["desc"])) for u in users.values()),
            "tell_outcomes": sorted({t["outcome"] for t in tells}), "tell_targets": sorted({t["target"] for t in tells if t["target"] is not None}),
            "speech_outcomes": sorted({speech_model(users[e[0]], e[1], e[2], e[3], True)["outcome"] for e in s["speak"]}),
            "read_kinds": sorted({answer_of(users[slot], data, False)[0]["kind"] for slot, data in s["reads"]})}


def footer_counts(users: dict) -> list:
    total = listed(users)
    invis = sum(not users[j]["vis"] for j in total)
    return [len(total) - invis, invis, len(total)]


# ------------------------------------------------------------------ comparing with the models
class Tally:
    """Comparisons made and differences found, part by part."""

    def __init__(self):
        self.comparisons, self.bad, self.counts, self.device_s = 0, [], {}, 0.0

    def add(self, what: str, n: int, bad) -> None:
        self.comparisons += n
        self.counts[what] = self.counts.get(what, 0) + n
        self.bad += [{"call": what, **b} for b in bad]

    def timed(self, call, *args, **kw):
        t0 = time.perf_counter()
        out = call(*args, **kw)
        self.device_s += time.perf_counter() - t0
        return out

    def result(self, **more) -> dict:
        return {"comparisons": self.comparisons, "by_call": self.counts, "n_bad": len(self.bad), "first_bad": self.bad[:3],
                "device_s": round(self.device_s, 3), **more}


def mirrors(roster: device.Roster):
    return roster._room.copy(), roster._flags.copy()


_CHUNKS: dict = {}


def chunks_of(text: bytes, c: int) -> list:
    if (text, c) not in _CHUNKS:
        _CHUNKS[text, c] = nuts_path.chunks(text, c)
    return _CHUNKS[text, c]


def plan_differences(plan: device.Plan, bs, room, flags):
    """A Plan against the predicate and the transducer: every bitmap word, the colour bits, both variants of every
    broadcast with their chunk sizes.  Returns the differences and the comparisons made."""
    bad = []
    want = admit_words(room, flags, bs)
    if plan.admitted_bits.shape != want.shape or plan.admitted_bits.dtype != np.uint64:
        bad.append({"what": "bitmap shape", "device": list(plan.admitted_bits.shape)})
    else:
        rows = np.flatnonzero((plan.admitted_bits != want).any(axis=1))
        if len(rows):
            k = int(rows[0])
            w = int(np.flatnonzero(plan.admitted_bits[k] != want[k])[0])
            bad.append({"what": "bitmap", "broadcast": k, "word": w, "device": hex(int(plan.admitted_bits[k, w])), "model": hex(int(want[k, w])),
                        "rows": len(rows)})
    if plan.colour_bits.tolist() != device._pack((flags & device.ROSTER_FLAGS["colour"]) != 0).tolist():
        bad.append({"what": "colour bits"})
    for k, b in enumerate(bs):
        for c in (0, 1):
            ch = chunks_of(b[0], c)
            n = int(plan.write_counts[k, c])
            if (plan.variant(k, c) != b"".join(ch) or n != len(ch) or plan.write_sizes[k, c, :n].tolist() != [len(x) for x in ch]
                    or int(plan.variant_sizes[k, c]) != sum(map(len, ch))):
                bad.append({"what": "variant", "broadcast": k, "colour": c, "device": [int(plan.variant_sizes[k, c]), n]})
                break
    return bad, want.size + 4 * len(bs) + 1


def fanout_differences(fo: device.Fanout, bs, room, flags, sample=None):
    """A Fanout against the predicate and the transducer: who is admitted, every item's size and chunk sizes through the
    offsets, the total, and the arena bytes of the admitted items (of ``sample`` alone, (k, slot) pairs, when given)."""
    bad = []
    cap, k = len(room), len(bs)
    want = device._unpack(admit_words(room, flags, bs), cap).reshape(k * cap)
    colour = ((flags & device.ROSTER_FLAGS["colour"]) != 0).astype(np.intp)
    var = [[b"".join(chunks_of(b[0], c)) for c in (0, 1)] for b in bs]
    wsz = [[[len(x) for x in chunks_of(b[0], c)] for c in (0, 1)] for b in bs]
    sizes = np.array([[len(v) for v in pair] for pair in var], dtype=np.int64)[:, colour].reshape(k * cap)
    writes = np.array([[len(w) for w in pair] for pair in wsz], dtype=np.int64)[:, colour].reshape(k * cap)
    out_off = np.concatenate([[0], np.cumsum(np.where(want, sizes, 0))])
    w_off = np.concatenate([[0], np.cumsum(np.where(want, writes, 0))])
    if not np.array_equal(fo.admitted, want):
        bad.append({"what": "admitted", "device": int(fo.admitted.sum()), "model": int(want.sum())})
    if not np.array_equal(fo.out_offsets, out_off) or len(fo.arena) != int(out_off[-1]):
        bad.append({"what": "out_offsets", "device": int(fo.out_offsets[-1]), "model": int(out_off[-1]), "arena": len(fo.arena)})
    if not np.array_equal(fo.write_offsets, w_off) or len(fo.write_sizes) != int(w_off[-1]):
        bad.append({"what": "write_offsets", "device": int(fo.write_offsets[-1]), "model": int(w_off[-1])})
    if not np.array_equal(fo.broadcast_offsets, np.arange(k + 1) * cap):
        bad.append({"what": "broadcast_offsets"})
    items = np.flatnonzero(want)
    if not bad:
        expect = np.concatenate([np.array(wsz[i // cap][colour[i % cap]], dtype=np.int32) for i in items.tolist()]
                                + [np.zeros(0, dtype=np.int32)])
        if not np.array_equal(fo.write_sizes, expect):
            bad.append({"what": "write_sizes"})
    checked = items.tolist() if sample is None else [kk * cap + j for kk, j in sample]
    if not bad:
        for i in checked:
            if fo.output(i) != (var[i // cap][colour[i % cap]] if want[i] else b""):
                bad.append({"what": "arena", "broadcast": i // cap, "slot": i % cap})
                break
    return bad, 2 * len(want) + int(w_off[-1]) + len(checked) + 3, len(checked), int(out_off[-1])


def speech_admit_differences(plan: device.Plan, users: dict, calls, room, flags):
    """The room lines of a Speech against the predicate: ``calls`` is, per event, None (not spoken) or ``(rm, sender, com)``."""
    bs = [(b"", None, None, 0, SAY) if c is None else (b"", c[0], c[1], 0, c[2]) for c in calls]
    want = admit_words(room, flags, bs)
    for k, c in enumerate(calls):
        if c is None:
            want[k] = 0
    rows = np.flatnonzero((plan.admitted_bits != want).any(axis=1))
    return [{"what": "room admitted", "event": int(rows[0])}] if len(rows) else [], want.size


def compare_speech(t: Tally, what: str, roster, users, events, ban, sp) -> None:
    room, flags = mirrors(roster)
    t.add(what, 6 * len(events), speech_differences(roster, users, events, ban, sp, {}, check_admits=False))
    models = [speech_model(users[e[0]], e[1], e[2], e[3], ban) for e in events]
    t.add(what, *speech_admit_differences(sp.room, users, [None if m["line"] is None else (m["rm"], m["sender"], e[1])
                                                            for m, e in zip(models, events)], room, flags)[::-1])


def compare_reads(t: Tally, what: str, roster, users, reads, ban, inp) -> None:
    room, flags = mirrors(roster)
    t.add(what, 8 * len(reads), input_differences(roster, users, reads, ban, inp, input_counts(), check_admits=False))
    answers = [answer_of(users[slot], data, ban) for slot, data in reads]
    t.add(what, *speech_admit_differences(inp.speech.room, users, [None if m["line"] is None else (m["rm"], m["sender"], d["com"])
                                                                   for d, m in answers], room, flags)[::-1])


def compare_review(t: Tally, what: str, rv: device.Review, rooms, rings, lines: int) -> int:
    """A Review or a revtell against its rings: every stored line, both variants, every chunk size."""
    bad, n = [], 0
    if rv.rooms.tolist() != list(rooms) or rv.stored.shape != (len(rooms), lines, device.REVIEW_LEN + 2):
        bad.append({"what": "rooms"})
    for q, rm in enumerate(rooms):
        want = rings.lines(rm)
        n += len(want)
        if rv.lines(q) != want or int(rv.line_counts[q]) != len(want):
            bad.append({"what": "lines", "ring": rm, "device": len(rv.lines(q)), "model": len(want)})
        for c in (0, 1):
            ch = rings.chunks(rm, c)
            k = int(rv.write_counts[q, c])
            if rv.chunks(q, c) != ch or rv.variant(q, c) != b"".join(ch) or rv.write_sizes[q, c, :k].tolist() != [len(x) for x in ch]:
                bad.append({"what": "variant", "ring": rm, "colour": c})
    t.add(what, 3 * len(rooms) + n, bad)
    return n


# ------------------------------------------------------------------ part 1: the edge roster
def edge_part() -> dict:
    t = Tally()
    t0 = time.perf_counter()
    users, rooms, records = edge_description()
    s = edge_script()
    names = {rm: r["name"] for rm, r in rooms.items()}
    rings, trings, cache = Rings(device.MAX_REVIEW_ROOMS), SparseTellRings(), {}
    shape = dict(capacity=CAPACITY, look_rooms=device.MAX_LOOK_ROOMS, review_rooms=device.MAX_REVIEW_ROOMS, revtell=True, clones=CAPACITY)
    roster = device.Roster(shape["capacity"], look_rooms=shape["look_rooms"], review_rooms=shape["review_rooms"], revtell=True,
                           clones=shape["clones"])
    seat_all(roster, users, rooms)
    seat_clones(roster, records)
    seen = {"relays_at_last_record": 0, "tell_outcomes": set(), "tell_targets": set(), "widest_pad": 0}

    def plans(bs, record=None):
        room, flags = mirrors(roster)
        plan = t.timed(roster.plan_many, bs, record=record)
        t.add("plan_many", *plan_differences(plan, bs, room, flags)[::-1])
        if record is not None:
            record_plan(rings, bs, record)
        fo = t.timed(roster.broadcast_many, bs)
        bad, n, _, _ = fanout_differences(fo, bs, room, flags)
        t.add("broadcast_many", n, bad)
        ex = plan.expand()
        same = all(np.array_equal(getattr(ex, f), getattr(fo, f)) for f in ("admitted", "out_offsets", "arena", "write_offsets", "write_sizes"))
        t.add("expand", 5, [] if same else [{"what": "plan.expand() differs from broadcast_many"}])

    def speaks(events, ban):
        sp = t.timed(roster.speak_many, events, ban_swearing=ban, record=True)
        compare_speech(t, "speak_many", roster, users, events, ban, sp)
        record_speech(rings, users, events, ban)

    def reads(rs):
        inp = t.timed(roster.input_many, rs, record=True)
        compare_reads(t, "input_many", roster, users, rs, False, inp)
        record_reads(rings, users, rs, False)

    def reviews(rms) -> int:
        rv = t.timed(roster.review_many, rms)
        t.add("review_many", len(rms), review_differences(rv, rms, rings, {"rooms_reviewed": 0, "lines_compared": 0, "sequential_lines": 0,
                                                                            "wave_lines": 0}, cache))
        compare_review(t, "review_many", rv, rms, rings, device.REVIEW_LINES)
        return len(rv.lines(0))

    def tells(events):
        pv = t.timed(roster.tell_many, events, record=True)
        t.add("tell_many", 8 * len(events), private_differences(roster, users, events, pv, tell_counts()))
        record_tells(trings, users, events)
        seen["tell_outcomes"] |= set(pv.outcome.tolist())
        seen["tell_targets"] |= set(pv.target.tolist()) - {-1}

    def revtells(slots) -> int:
        rv = t.timed(roster.revtell_many, slots)
        compare_review(t, "revtell_many", rv, slots, trings, device.REVTELL_LINES)
        return len(rv.lines(0))

    def looks(slots):
        lk = t.timed(roster.look_many, slots)
        t.add("look_many", sum(3 + len(members(users, j)) for j in slots), look_differences(users, rooms, slots, lk, look_counts()))

    def whos(slots):
        w = t.timed(roster.who_many, slots, now=NOW, date=DATE)
        t.add("who_many", 2 + 3 * (4 + len(listed(users))) + 3 * len(slots), who_differences(users, rooms, slots, NOW, DATE, w, who_counts()))
        seen["widest_pad"] = max([seen["widest_pad"]] + [w.text(4 + l).index(b" : ") for l in range(len(w.line_slots))])

    def relay(bs, record, csenders):
        room, flags = mirrors(roster)
        rl = t.timed(roster.relay_many, bs, record=record, clone_sender=csenders)
        t.add("relay_many", 6 * len(bs), relay_differences(roster, users, records, bs, csenders or [None] * len(bs), rl, relay_counts(),
                                                           names))
        t.add("relay_many", *plan_differences(rl.plan, bs, room, flags)[::-1])
        if record is not None:
            record_plan(rings, bs, record)
        seen["relays_at_last_record"] += sum(LAST in rl.relays(k).tolist() for k in range(len(bs)))

    with roster:
        plans(s["plan"], s["plan_record"])
        speaks(s["speak"], True)
        reads(s["reads"])
        ring_lines = reviews(s["review"])
        tells(s["tell"])
        revtell_lines = revtells(s["revtell"])
        roster.clear_revtell(LAST)
        trings.clear(LAST)
        cleared = revtells([LAST, 0])
        looks(s["look"])
        whos(s["who"])
        relay(s["relay"], s["relay_record"], s["relay_clone_sender"])
        # slot 65,535, record 65,535 and room 1,023 alone: the re-upload and the copy blocks carry each table's last words
        edge_update(users, rooms, records)
        apply_edge_update(roster, users, rooms, records)
        names = {rm: r["name"] for rm, r in rooms.items()}
        relay(s["again_relay"], None, None)
        whos(s["who"])
        looks(s["look"])
        tells(s["again_tell"])
        speaks(s["again_speak"], False)
        reads(s["again_reads"])
        plans(s["again_plan"])
        reviews(s["review"])
        revtells(s["revtell"])
    return t.result(roster=shape, slots=len(users), ring_last_room=ring_lines, revtell_last=revtell_lines, revtell_after_clear=cleared,
                    relays_at_last_record=seen["relays_at_last_record"], tell_outcomes=sorted(seen["tell_outcomes"]),
                    tell_targets=sorted(seen["tell_targets"]), widest_pad=seen["widest_pad"], wall_s=round(time.perf_counter() - t0, 3))


# ------------------------------------------------------------------ part 2: the full roster
def who_full_differences(users: dict, rooms: dict, slots, w: device.Who):
    """A Who of tens of thousands of lines against ``who_line`` and the transducer: every text, both variants and their chunk
    sizes as whole buffers, each looker's bitmap word by word, each looker's output."""
    bad, order = [], listed(users)
    nl = len(order)
    fixed = who(users, rooms, slots[0], NOW, DATE)
    strings = [b"\n*** Current users %s ***\n\n" % DATE, b"\n~BB*** Current users %s ***\n\n" % DATE, fixed[-2], fixed[-1]]
    strings += [who_line(users[j], rooms, NOW) for j in order]
    if w.line_slots.tolist() != order:
        bad.append({"what": "line_slots"})
    if len(w.text_sizes) != len(strings) or w.text_sizes.tolist() != [len(x) for x in strings]:
        bad.append({"what": "text sizes", "device": len(w.text_sizes), "model": len(strings)})
    elif device._gather(w.texts, w.text_starts, w.text_sizes).tobytes() != b"".join(strings):
        bad.append({"what": "texts"})
    ch = [[nuts_path.chunks(x, c) for x in strings] for c in (0, 1)]
    var = [[b"".join(x) for x in ch[c]] for c in (0, 1)]
    for c in (0, 1):
        sizes = np.array([len(x) for x in var[c]], dtype=np.int64)
        counts = np.array([len(x) for x in ch[c]], dtype=np.int64)
        if bad or not np.array_equal(w.variant_sizes[:, c], sizes) or not np.array_equal(w.write_counts[:, c], counts):
            bad.append({"what": "variant sizes", "colour": c})
            continue
        if device._gather(w.variants, w.variant_starts[:, c].copy(), sizes).tobytes() != b"".join(var[c]):
            bad.append({"what": "variants", "colour": c})
        want = np.concatenate([np.array([len(y) for y in x], dtype=np.int32) for x in ch[c]])
        got = w.write_sizes[:, c, :][np.arange(device.MAX_WRITES)[None, :] < counts[:, None]]
        if not np.array_equal(got, want):
            bad.append({"what": "write sizes", "colour": c})
    words = max(1, -(-nl // 32))
    shown_lines = 0
    position = {j: l for l, j in enumerate(order)}
    for k, slot in enumerate(slots):
        see = np.zeros(32 * words, dtype=bool)
        lines = [position[j] for j in shown(users, slot)]
        see[lines] = True
        shown_lines += len(lines)
        u = users[slot]
        if w.shown.shape != (len(slots), words) or not np.array_equal(w.shown[k], np.packbits(see, bitorder="little").view("<u4")):
            bad.append({"what": "shown", "who": k})
        elif not bad:
            c = int(u["colour"])
            head = device.WHO_HEAD_LOGIN if u["login"] else device.WHO_HEAD
            want = [x for t_ in [head] + [4 + l for l in lines] + [device.WHO_FOOT, device.WHO_TAIL] for x in ch[c][t_]]
            if w.chunks(k) != want or int(w.colour[k]) != c or int(w.login[k]) != u["login"]:
                bad.append({"what": "chunks", "who": k})
    return bad, {"lines": nl, "texts": len(strings), "bitmap_words": len(slots) * words, "shown_lines": shown_lines,
                 "footer": strings[device.WHO_FOOT].decode()}


def full_part() -> dict:
    t = Tally()
    t0 = time.perf_counter()
    users, rooms = full_description()
    roster = device.Roster(CAPACITY, look_rooms=2)
    seat_all(roster, users, rooms)
    model_s = {"describe": round(time.perf_counter() - t0, 3)}
    out = {}
    gathers = []
    real_gather = device._gather

    def counting(src, starts, counts, step=1 << 24):
        ends, lo, at, steps = np.cumsum(counts), 0, 0, 0
        while lo < len(counts):                             # _gather's own partition: how many runs it takes
            lo = max(int(np.searchsorted(ends, at + step, side="right")), lo + 1)
            at, steps = int(ends[lo - 1]), steps + 1
        gathers.append(steps)
        return real_gather(src, starts, counts, step)

    with roster:
        # who: tens of thousands of lines, five-digit counts, 256 tiles per looker
        w = t.timed(roster.who_many, list(FULL_WHO_LOOKERS), now=NOW, date=DATE)
        t1 = time.perf_counter()
        bad, info = who_full_differences(users, rooms, list(FULL_WHO_LOOKERS), w)
        model_s["who"] = round(time.perf_counter() - t1, 3)
        t.add("who_many", 5 * info["texts"] + info["bitmap_words"] + info["shown_lines"], bad)
        out["who"] = {**info, "device_footer": w.text(device.WHO_FOOT).decode(), "lookers": list(FULL_WHO_LOOKERS)}
        del w
        # look: member lists and line ranges of tens of thousands
        lk = t.timed(roster.look_many, list(FULL_LOOKERS))
        t1 = time.perf_counter()
        n_members = [len(members(users, j)) for j in FULL_LOOKERS]
        t.add("look_many", sum(n_members) + 6 * len(FULL_LOOKERS), look_differences(users, rooms, list(FULL_LOOKERS), lk, look_counts()))
        population = [sum(1 for u in users.values() if u["room"] == users[j]["room"]) for j in FULL_LOOKERS]
        taken = [int((lk.line_slots[int(a):int(a) + p] >= 0).sum()) for a, p in zip(np.cumsum([0] + population[:-1]), population)]
        if taken != population or len(lk.line_slots) != sum(population):
            t.add("look_many", 0, [{"what": "line ranges", "device": taken, "model": population}])
        model_s["look"] = round(time.perf_counter() - t1, 3)
        out["look"] = {"members": lk.member_counts.tolist(), "model_members": n_members, "lines": population, "lookers": list(FULL_LOOKERS)}
        del lk
        # tell: get_user over every slot
        first, second = full_tell_cases()
        t1 = time.perf_counter()
        out["tell"] = {}
        for cases in (first, second):
            events = [c[1] for c in cases]
            pv = t.timed(roster.tell_many, events)
            t.add("tell_many", 8 * len(events), private_differences(roster, users, events, pv, tell_counts()))
            out["tell"].update({c[0]: [int(pv.outcome[k]), int(pv.target[k])] for k, c in enumerate(cases)})
            if cases is first:
                slots, new = full_renames()
                for j, name in zip(slots, new):
                    users[j]["name"] = name
                roster.update(slots, name=new)
        model_s["tell"] = round(time.perf_counter() - t1, 3)
        # plan: 8 broadcasts against the predicate
        room, flags = mirrors(roster)
        bs = [(b"to the hall\n", 0, 0, 0, SAY), (b"~OLU32768 shouts:~RS hear me\n", None, 32768, 0, SHOUT), (b"to the annexe\n", 1, LAST, 0, SAY),
              (b"~OL!!~RS everyone\n", None, None, 0, SEMOTE), (b"forced on the hall\n", 0, None, 1, SAY), (b"forced shout\n", None, 0, 1, SHOUT),
              (b"", 1, 32768, 0, EMOTE), (b"nobody's room\n", 2, LAST, 0, SAY)]
        plan = t.timed(roster.plan_many, bs)
        t1 = time.perf_counter()
        bad, n = plan_differences(plan, bs, room, flags)
        t.add("plan_many", n, bad)
        model_s["plan"] = round(time.perf_counter() - t1, 3)
        out["plan"] = {"broadcasts": len(bs), "bitmap_words": int(plan.admitted_bits.size),
                       "admitted": [int(np.unpackbits(plan.admitted_bits[k].view(np.uint8)).sum()) for k in range(len(bs))]}
        # broadcast: two short texts to everyone
        two = [(b"~FRA short line~RS to the whole hall, " + b"with some /~FG words " * 10 + b"to fill it.\n", 0, 0, 0, SAY),
               (b"~OLU65535 shouts:~RS " + b"every slot hears this; " * 12 + b"\n", None, LAST, 0, SHOUT)]
        fo = t.timed(roster.broadcast_many, two)
        t1 = time.perf_counter()
        rng = random.Random(7)
        admitted = [np.flatnonzero(fo.admitted[k * CAPACITY:(k + 1) * CAPACITY]) for k in range(2)]
        sample = [(k, int(a[0])) for k, a in enumerate(admitted)] + [(k, int(a[-1])) for k, a in enumerate(admitted)]
        sample += [(k, int(rng.choice(admitted[k].tolist()))) for k in (0, 1) for _ in range(32)]
        sample += [(0, 0), (1, LAST)]                       # the senders: not admitted, no bytes
        bad, n, checked, total = fanout_differences(fo, two, room, flags, sample)
        t.add("broadcast_many", n, bad)
        device._gather = counting
        try:
            ex = roster.plan_many(two).expand()
        finally:
            device._gather = real_gather
        same = all(np.array_equal(getattr(ex, f), getattr(fo, f)) for f in ("admitted", "out_offsets", "arena", "write_offsets", "write_sizes"))
        t.add("expand", 5, [] if same else [{"what": "plan.expand() differs from broadcast_many"}])
        model_s["broadcast"] = round(time.perf_counter() - t1, 3)
        out["broadcast"] = {"arena_bytes": int(fo.out_offsets[-1]), "model_bytes": total, "arena_items_compared": checked,
                            "arena_bound": int((roster._room >= 0).sum()) * sum(device.max_bytes(len(b[0])) for b in two)}
        del fo, ex
        # part 3: the accept side of the size guards
        rng = random.Random(11)
        many = [(rng.choice(GUARD_LINES), rng.choice((0, 1, None, 2)), rng.choice((None, 0, 255, 256, 32768, LAST, rng.randrange(CAPACITY))),
                 rng.randrange(2), rng.choice((SAY, SHOUT, EMOTE, SEMOTE))) for _ in range(GUARD_K)]
        g = Tally()
        plan = g.timed(roster.plan_many, many)
        t1 = time.perf_counter()
        bad, n = plan_differences(plan, many, room, flags)
        g.add("plan_many", n, bad)
        guards = g.result(k=GUARD_K, cells=GUARD_K * CAPACITY, bitmap_words=int(plan.admitted_bits.size), distinct_lines=len(GUARD_LINES),
                          model_s=round(time.perf_counter() - t1, 3), gather_steps={"expand_of_part_2": gathers})
    return {"full": t.result(roster={"capacity": CAPACITY, "look_rooms": 2}, model_s=model_s, wall_s=round(time.perf_counter() - t0, 3), **out),
            "guards": guards}


def main() -> int:
    if device.device_count() < 1:
        print("no GPU visible", file=sys.stderr)
        return 3
    t0 = time.perf_counter()
    res = {"edge": edge_part(), **full_part()}
    res["wall_s"] = round(time.perf_counter() - t0, 3)
    res["device_s"] = round(sum(res[part]["device_s"] for part in ("edge", "full", "guards")), 3)      # inside the Roster's calls
    res["model_s"] = round(res["wall_s"] - res["device_s"], 3)                                         # the models and the comparing
    print("DEVICE_LIMITS " + json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
