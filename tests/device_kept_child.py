"""The device work of tests/test_device_kept.py, in a short-lived child process of its own.

As tests/device_sequence_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_KEPT {...}``).  A roster keeps eight tables on the device between calls -- the speaker state, the
AFK messages, the room table, the users' descriptions, the who table, the clone records, the relay's room names and the go
table -- and a call passes one only when it changed.  The other children sample that at random.  This one makes, for every
call kind that reads kept tables, every subset of them the one that is passed: 56 cases.  A case changes exactly the tables
of its subset, each at both ends and through a field the call's output shows, makes the call (the kernel reads the uploads
and its copy tail fills the kept allocations), and makes it again with nothing passed (the kernel reads the kept allocations
alone).  ``go_many`` cannot be made twice, and only a move shows its tables: it has a runner of its own, ``run_go``.

The roster has 65 slots, 3 look rooms and 3 clone records: the boundaries between the tables fall inside a 256-thread
block of the copy tail, the tail is longer than one block, and its last block is partial.

    python tests/device_kept_child.py
"""
from __future__ import annotations

import dataclasses
import itertools
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from device_go_child import go_call, go_differences, mirror_differences, population  # noqa: E402
from device_input_child import input_differences  # noqa: E402
from device_input_child import new_counts as input_counts  # noqa: E402
from device_look_child import look_differences  # noqa: E402
from device_look_child import new_counts as look_counts  # noqa: E402
from device_relay_child import ALL, SWEARS, put_records, relay_differences  # noqa: E402
from device_relay_child import new_counts as relay_counts  # noqa: E402
from device_rooms_child import list_room, rooms_differences  # noqa: E402
from device_speak_child import EMOTE, SAY, speech_differences  # noqa: E402
from device_tell_child import TELL, new_user, private_differences  # noqa: E402
from device_tell_child import new_counts as tell_counts  # noqa: E402
from device_who_child import new_counts as who_counts  # noqa: E402
from device_who_child import who_differences  # noqa: E402
from nuts333_amd import device  # noqa: E402

CAPACITY, LOOK_ROOMS, CLONES = 65, 3, 3
NOW, DATE = 1_000_000, b"DATE"
#: each kind's kept tables, in the order its layout places their uploads
TABLES = {"speak_many": ("speech",), "input_many": ("speech",), "tell_many": ("speech", "afk"),
          "look_many": ("speech", "rooms", "udesc"), "who_many": ("speech", "rooms", "udesc", "who"),
          "rooms_many": ("speech", "rooms"), "relay_many": ("names", "clones"), "go_many": ("speech", "clones", "rooms", "go")}
#: the kinds whose case is one call made twice, byte for byte; go_many's cases are run_go's
TWICE = tuple(k for k in TABLES if k != "go_many")
SEATED = {0: 0, 1: 0, 2: 0, 31: 0, 33: 2, 62: 2, 63: 2, 64: 2}          # slot -> room
#: rooms_many shows of the speaker state only whether a slot has a name, and a name cannot be taken back: its two cases
#: that pass the speaker state name a pair of slots each, the outermost pair in the case that passes it alone
NAMELESS = ((0, 64), (2, 62))
USER_FIELDS = ("room", "login", "ignall", "ignshout", "colour", "vis", "muzzled", "command_mode", "level", "afk", "igntell", "afk_mesg",
               "desc", "last_login")
ROOM_FIELDS = ("name", "access", "desc", "links", "topic", "mesg_cnt", "netlink", "inlink")


def subsets(tables) -> list:
    return [c for n in range(len(tables) + 1) for c in itertools.combinations(tables, n)]


class State:
    """The truth in plain Python, as the models of the other children read it, and the updates that change one kept
    table each, at both of its ends."""

    def __init__(self, kind: str):
        self.kind, self.n = kind, {}
        self.users = {j: new_user(j, room=None, ignshout=0, desc=b"", last_login=0, away=None, prompt=0, in_phrase=b"enters",
                                  out_phrase=b"goes", invite=None) for j in range(CAPACITY)}
        for j, rm in SEATED.items():
            self.users[j].update(room=rm, name=b"User%02d" % j, colour=j % 2, level=3, desc=b"is slot %d" % j, last_login=NOW - 60 * j)
        for j in (0, 64):                                               # the targets of tell_many's AFK replies
            self.users[j].update(afk=1, afk_mesg=b"away %d" % j)
        if kind == "rooms_many":
            for j in itertools.chain(*NAMELESS):
                self.users[j]["name"] = None
        self.rooms = [list_room(b"hall", desc=b"A hall.\n", links=[1], topic=b"halls", mesg_cnt=3),
                      list_room(b"mid", access=device.PRIVATE, links=[0, 2]),
                      list_room(b"attic", desc=b"An attic.\n", topic=b"attics", netlink=(b"far", False), inlink=True)]
        self.records = [[1, 0, ALL], [None, None, 0], [63, 2, SWEARS]]
        if kind == "go_many":
            # the rooms at both ends exactly PRIVATE, so that leaving one counts who stays behind, the clone records too, and
            # every room linked to the other two, so that a walk shows the phrases; the records start in the middle room
            self.rooms[0].update(access=device.PRIVATE, links=[1, 2])
            self.rooms[1].update(access=device.PUBLIC)
            self.rooms[2].update(access=device.PRIVATE, links=[0, 1])
            self.records[0][1] = self.records[2][1] = 1

    def seat(self, roster: device.Roster) -> None:
        for j in SEATED:
            u = self.users[j]
            roster.update(j, **{f: u[f] for f in USER_FIELDS}, **({"name": u["name"]} if u["name"] else {}))
        ids = list(range(LOOK_ROOMS))
        roster.set_rooms(ids, **{f: [self.rooms[i][f] for i in ids] for f in ROOM_FIELDS})
        if self.kind in ("relay_many", "go_many"):
            put_records(roster, self.records)
        if self.kind == "go_many":
            for j in SEATED:
                u = self.users[j]
                roster.update(j, in_phrase=u["in_phrase"], out_phrase=u["out_phrase"], invite_room=u["invite"])

    def change(self, roster: device.Roster, table: str) -> None:
        n = self.n[table] = self.n.get(table, 0) + 1
        ends = (0, 64)
        if table == "speech":
            if self.kind == "rooms_many":
                ends = NAMELESS[1] if self.users[NAMELESS[0][0]]["name"] else NAMELESS[0]
            names = [b"Ann%02d" % n, b"Zed%02d" % n]
            roster.update(list(ends), name=names)
            for j, v in zip(ends, names):
                self.users[j]["name"] = v
        elif table in ("afk", "udesc", "who"):
            field = {"afk": "afk_mesg", "udesc": "desc", "who": "last_login"}[table]
            values = [NOW - 3600 * n, NOW - 7200 * n] if table == "who" else [b"%s %02d a" % (table.encode(), n), b"%s %02d z" % (table.encode(), n)]
            roster.update(list(ends), **{field: values})
            for j, v in zip(ends, values):
                self.users[j][field] = v
        elif table in ("rooms", "names"):
            new = {"name": [b"hall%02d" % n, b"attic%02d" % n]}
            if table == "rooms":
                new.update(topic=[b"topic %02d a" % n, b"topic %02d z" % n], desc=[b"A hall, %02d.\n" % n, b"An attic, %02d.\n" % n])
            roster.set_rooms([0, 2], **new)
            for f, values in new.items():
                self.rooms[0][f], self.rooms[2][f] = values
        elif table == "go":
            # the phrases a walk shows.  An invite that lets a mover into a private room is dropped by the move, and the next
            # call would pass the go table again: the invite changes with the phrases, into the middle room, where nobody
            # goes, and nothing shows it but the mirrors and the fresh roster
            ins, outs = [b"in %02d a" % n, b"in %02d z" % n], [b"out %02d a" % n, b"out %02d z" % n]
            invite = 1 if n % 2 else None
            roster.update(list(ends), in_phrase=ins, out_phrase=outs, invite_room=invite)
            for j, i, o in zip(ends, ins, outs):
                self.users[j].update(in_phrase=i, out_phrase=o, invite=invite)
        elif self.kind == "go_many":
            # the clone records at both ends: into the rooms at both ends, where each keeps the room that a mover leaves
            # private, and back into the middle room.  A record that the device still saw in the middle room would let the
            # room return to public; one it still saw at an end shows nothing, so the way back only sets the next case up
            rooms = [0, 2] if n % 2 else [1, 1]
            roster.set_clones([0, 2], room=rooms)
            self.records[0][1], self.records[2][1] = rooms
        else:                                                           # the clone records: who hears what
            for c in (0, 2):
                self.records[c][2] = SWEARS if self.records[c][2] == ALL else ALL
                roster.set_clones(c, hear=self.records[c][2])


# ------------------------------------------------------------------ the request of each kind, from the state as it is now
def request(kind: str, st: State):
    u = st.users
    if kind == "speak_many":
        return [(0, SAY, b"hello there", 3), (64, EMOTE, b"waves about", 3), (1, SAY, b"hi", 2)]
    if kind == "input_many":
        return [(0, b"hello there\n"), (64, b".emote waves about\n"), (33, b"hi\n")]
    if kind == "tell_many":
        return [(1, TELL, u[64]["name"] + b" are you there", 5), (33, TELL, u[0]["name"] + b" hello?", 3), (0, TELL, u[1]["name"] + b" a told line", 5)]
    if kind == "relay_many":
        return [(b"a plain line\n", 0, None, 0, 0), (b"a shit line\n", 0, 31, 0, 0), (b"a plain line\n", 2, None, 0, 0), (b"a shit line\n", 2, 33, 1, 0),
                (b"elsewhere\n", 1, None, 0, 0)]
    if kind == "go_many":
        return go_walks(st)[0]
    return {"look_many": [1, 33, 0, 64], "who_many": [0, 64], "rooms_many": [1, 33]}[kind]


def call(kind: str, roster: device.Roster, req):
    if kind in ("speak_many", "input_many", "tell_many", "relay_many", "look_many"):
        return getattr(roster, kind)(req)
    if kind == "who_many":
        return roster.who_many(req, now=NOW, date=DATE)
    return roster.rooms_many(req, topics=[True, False])


def differences(kind: str, roster: device.Roster, st: State, req, got) -> list:
    """What of the result differs from the model of the child that owns the kind."""
    if kind == "speak_many":
        return speech_differences(roster, st.users, req, False, got, {})
    if kind == "input_many":
        return input_differences(roster, st.users, req, False, got, input_counts())
    if kind == "tell_many":
        return private_differences(roster, st.users, req, got, tell_counts())
    if kind == "look_many":
        return look_differences(st.users, st.rooms, req, got, look_counts())
    if kind == "who_many":
        return who_differences(st.users, st.rooms, req, NOW, DATE, got, who_counts())
    if kind == "rooms_many":
        seen = {"colours": set(), "empty": 0, "single": 0, "all": 0, "uncounted": 0, "nameless_rooms": 0, "states": set(), "inlinks": set(),
                "fixed": 0}
        return rooms_differences(st.users, st.rooms, req, [True, False], got, seen)
    names = {i: rm["name"] for i, rm in enumerate(st.rooms)}
    return relay_differences(roster, st.users, [tuple(r) for r in st.records], req, [None] * len(req), got, relay_counts(), names=names)


# ------------------------------------------------------------------ what a result holds
def arrays(result, prefix="") -> dict:
    """Every array of a result as its bytes, the nested plans' too: what two calls on one allocation return alike, the
    unspecified gaps included."""
    out = {}
    for f in dataclasses.fields(result):
        v = getattr(result, f.name)
        if isinstance(v, np.ndarray):
            out[prefix + f.name] = v.tobytes()
        elif dataclasses.is_dataclass(v):
            out.update(arrays(v, prefix + f.name + "."))
    return out


def plan_says(p: device.Plan, k: int) -> list:
    return [p.admitted(k).tolist()] + [p.chunks(k, c) for c in (0, 1)]


def says(kind: str, got, k: int) -> list:
    """What the result says about entry ``k``, read through its own accessors: what a fresh roster must return as well."""
    if kind == "input_many":
        return [int(got.kind[k]), int(got.com[k]), got.inpstr(k), got.line(k)] + says("speak_many", got.speech, k)
    if kind == "speak_many":
        return [int(got.outcome[k]), got.line(k), got.reply_text(k)] + plan_says(got.room, k) + plan_says(got.reply, k)
    if kind == "tell_many":
        return [int(got.outcome[k]), int(got.target[k]), got.line(k), got.reply_text(k)] + plan_says(got.told, k) + plan_says(got.reply, k)
    if kind == "relay_many":
        return plan_says(got.plan, k) + [got.relays(k).tolist(), got.owners(k).tolist(), got.relay_text(k)] + [got.relay_chunks(k, c) for c in (0, 1)]
    extra = {"look_many": lambda: got.members(k).tolist(), "who_many": lambda: got.lines(k).tolist(), "rooms_many": lambda: got.counts.tolist()}
    return [got.output(k), got.chunks(k), [got.text(t) for t in got.text_numbers(k)], extra[kind]()]


def all_says(kind: str, got, n: int) -> list:
    return [says(kind, got, k) for k in range(n)]


# ------------------------------------------------------------------ the flags, and the sizes the upload is made of
def passed(kind: str, roster: device.Roster, req) -> list:
    """The kept tables of ``kind`` that the roster's private flags say its next call passes."""
    flag = {"speech": roster._speech_dirty or (kind in ("tell_many", "look_many", "who_many") and roster._private_dirty),
            "afk": roster._afk_dirty, "rooms": roster._rooms_dirty, "udesc": roster._udesc_dirty, "who": roster._who_dirty,
            "clones": roster._clones_dirty, "go": roster._go_dirty}
    if kind == "relay_many":
        names = roster._prepare_relay(req, None, None)[2]
        flag["names"] = roster._relay_names is None or not np.array_equal(names, roster._relay_names)
    return [t for t in TABLES[kind] if flag[t]]


def table_slices(roster: device.Roster) -> dict:
    """The arrays each kept table's upload is made of, in bytes, from the mirrors the module keeps (the clone records go up
    as three arrays, the relay's names as 24 bytes per look room)."""
    return {"speech": [roster._speech.nbytes], "afk": [roster._afk.nbytes], "rooms": [roster._rooms.nbytes], "udesc": [roster._udesc.nbytes],
            "who": [roster._who.nbytes], "names": [24 * roster.look_rooms], "go": [roster._go.nbytes],
            "clones": [roster._clone_owner.nbytes, roster._clone_room.nbytes, roster._clone_hear.nbytes]}


def input_arrays(kind: str, req, st: State) -> list:
    """The arrays of a call's own inputs, in bytes: a call that passes no table uploads these, a 256-byte aligned slice each,
    and the violation count's four bytes."""
    k = len(req)
    if kind in ("speak_many", "tell_many"):                             # the texts, their offsets and lengths, the slots, the commands,
        return [sum(len(e[2]) for e in req), 4 * k, 4 * k, 4 * k, k, k, 8 * k]   # the word counts, the composed texts' offsets
    if kind == "input_many":                                            # the reads, their offsets and lengths, the slots, the offsets
        return [sum(len(d) for _, d in req), 4 * k, 4 * k, 4 * k, 8 * k]
    if kind == "relay_many":                                            # the texts; seven int32 per broadcast; the flag bytes
        return [sum(len(b[0]) for b in req)] + [4 * k] * 7 + [k]
    if kind == "who_many":                                              # the lookers, the date's 80 bytes
        return [4 * k, 80]
    if kind == "rooms_many":
        return [4 * k]
    if kind == "go_many":                                               # the lines, their offsets and lengths, the movers, the word
        return [sum(len(e[1]) for e in req), 4 * k, 4 * k, 4 * k, k, 16 * k]     # counts, the four texts' offsets per event
    rooms = {st.users[j]["room"] for j in req}                          # look_many: the lookers, their rooms, the distinct rooms, the
    nr = len(rooms)                                                     # rooms' line ranges, the lookers' member ranges, the texts' offsets
    nl = sum(1 for u in st.users.values() if u["room"] in rooms)
    return [4 * k, 4 * k, 4 * nr, 4 * (nr + 1), 4 * (k + 1), 4 * (5 * nr + 3 + nl)]


def new_roster(st: State) -> device.Roster:
    roster = device.Roster(CAPACITY, look_rooms=LOOK_ROOMS, clones=CLONES if st.kind in ("relay_many", "go_many") else 0)
    st.seat(roster)
    return roster


def run_kind(kind: str) -> list:
    st = State(kind)
    roster = new_roster(st)
    call(kind, roster, request(kind, st))                               # primed: everything was passed
    out = []
    for subset in subsets(TABLES[kind]):
        for table in subset:
            st.change(roster, table)
        req = request(kind, st)
        case = {"kind": kind, "subset": list(subset), "flags": passed(kind, roster, req), "table_dirty": bool(roster._dirty),
                "inputs": input_arrays(kind, req, st)}
        first = call(kind, roster, req)                                 # reads the uploads
        case["flags_after"] = passed(kind, roster, req)
        again = call(kind, roster, req)                                 # reads the kept tables alone
        fresh_roster = new_roster(st)
        fresh = call(kind, fresh_roster, req)                           # the final state, everything passed
        fresh_roster.close()
        a, b = arrays(first), arrays(again)
        case["h2d"] = [first.timing["h2d_bytes"], again.timing["h2d_bytes"]]
        case["d2h"] = [first.timing["d2h_bytes"], again.timing["d2h_bytes"]]
        case["arrays"] = len(a)
        case["arrays_differ"] = sorted(name for name in a if a[name] != b[name])
        said = all_says(kind, first, len(req))
        case["again_says_the_same"] = all_says(kind, again, len(req)) == said
        case["fresh_says_the_same"] = all_says(kind, fresh, len(req)) == said
        case["model_differences"] = [differences(kind, roster, st, req, r)[:2] for r in (first, again)]
        out.append(case)
    sizes = table_slices(roster)
    roster.close()
    return [{**c, "tables": {t: sizes[t] for t in TABLES[kind]}} for c in out]


# ------------------------------------------------------------------ go_many: two different calls, both of them moves
GATECRASH = 3                                                           # the level of every seated slot: the private rooms admit them


def go_walks(st: State) -> list:
    """The two calls of a round, from where slots 0 and 64 stand: the one in room 0 walks into room 2, then the other walks
    from room 2 into room 0.  With three rooms a call holds one move -- a move touches two rooms, and an event in a touched
    room is deferred -- so each call's other event is the other end's, asking for the room it stands in: the two ends swap
    places in a round, and a case is two rounds.  The words are what the rooms' names begin with, whatever they are now."""
    first = 0 if st.users[0]["room"] == 0 else 64
    other = 64 - first
    return [[(other, b"attic", 2), (first, b" attic now", 3)], [(first, b"attic", 2), (other, b"hall", 2)]]


def go_clones(st: State) -> list:
    return [None if r[0] is None else tuple(r) for r in st.records]


def go_says(got: device.Go) -> list:
    """What a Go says, read through its own accessors: what a fresh roster in the same state must return as well."""
    plans = (got.enter, got.leave, got.reset, got.reply)
    out = [[int(got.outcome[k]), int(got.target[k]), int(got.old_room[k]), bool(got.returned_public[k]), got.enter_text(k),
            got.leave_text(k), got.reset_text(k), got.reply_text(k)] + [x for p in plans for x in plan_says(p, k)]
           for k in range(len(got.outcome))]
    return out + [None if got.look is None else [got.look.chunks(i) for i in range(len(got.look.slots))]]


def go_flags(roster: device.Roster) -> list:
    return passed("go_many", roster, None) + (["table"] if roster._dirty else [])


def run_go() -> list:
    """go_many's 16 cases.  A case is two rounds; a round changes the tables of the subset and makes two calls.  The first
    call's kernel reads the uploads, the second's the kept allocations the first call's tail filled; both walk, so both show
    the names, the phrases, the rooms' names and who keeps the room left private.  ``min_private_users`` is exactly who stays
    behind, clone records included, so no room returns to public: the first call leaves the table dirty and nothing else,
    its own look uploads that, and the second call passes nothing."""
    kind = "go_many"
    st = State(kind)
    roster = new_roster(st)

    def walk(events) -> dict:
        mover = events[1][0]
        stay = population(st.users, go_clones(st), st.users[mover]["room"], mover)
        fresh_st = State(kind)                                          # a fresh roster seated in the state this call meets
        fresh_st.users, fresh_st.rooms = {j: dict(u) for j, u in st.users.items()}, [dict(rm) for rm in st.rooms]
        fresh_st.records = [list(r) for r in st.records]
        fresh_roster = new_roster(fresh_st)
        fresh = fresh_roster.go_many(events, gatecrash_level=GATECRASH, min_private_users=stay)
        fresh_roster.close()
        model = go_call(st.users, st.rooms, go_clones(st), events, GATECRASH, stay)                  # the state moves
        got = roster.go_many(events, gatecrash_level=GATECRASH, min_private_users=stay)
        bad = go_differences(got, model, st.users, st.rooms) + mirror_differences(roster, st.users, st.rooms)
        return {"inputs": input_arrays(kind, events, st), "h2d": got.timing["h2d_bytes"],
                "look_h2d": got.look.timing["h2d_bytes"] if got.look is not None else None, "flags_after": go_flags(roster),
                "outcomes": got.outcome.tolist(), "returned": got.returned_public.tolist(), "stay": stay,
                "model_differences": bad[:2], "fresh_says_the_same": go_says(fresh) == go_says(got)}

    # primed with two rounds of the same walks: everything was passed, and the allocation has held a call of two events and
    # its look, so that no case meets it made anew and uploads the table for that
    primed = [walk(events) for _ in range(2) for events in go_walks(st)]
    out = []
    for subset in subsets(TABLES[kind]):
        case = {"kind": kind, "subset": list(subset), "rounds": []}
        for _ in range(2):
            for table in subset:
                st.change(roster, table)
            flags = go_flags(roster)
            case["rounds"].append({"flags": flags, "calls": [walk(events) for events in go_walks(st)]})
        out.append(case)
    out[0]["primed"] = [not c["model_differences"] and c["fresh_says_the_same"] for c in primed]
    sizes = table_slices(roster)
    roster.close()
    return [{**c, "tables": {t: sizes[t] for t in TABLES[kind]}} for c in out]


def main() -> int:
    if device.device_count() < 1:
        print("no GPU visible", file=sys.stderr)
        return 3
    cases = [c for kind in TWICE for c in run_kind(kind)] + run_go()
    print("DEVICE_KEPT " + json.dumps({"cases": cases, "order": {k: list(v) for k, v in TABLES.items()}}, default=str))
    return 0


if __name__ == "__main__":
    sys.exit(main())
