"""The device work of tests/test_device_rooms.py, in a short-lived child process of its own, and the CPU model the host
tier of that module shares with it.

As tests/device_who_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_ROOMS {...}``).  ``rooms`` is the Python model of ``rooms(user, show_topics)``
(nuts333.c:5661-5700), built from the reference's format strings: the strings of its ``write_user`` calls, in order.
``replay_listings`` runs the recorded session tests/golden/reference_only/rmst.json: accounts are seated as they log in,
``.go``, ``.topic``, ``.write``, ``.private`` and ``.invis`` are applied, and the bytes of every ``.rmst`` and ``.rmsn``
are compared with the answer.

    python tests/device_rooms_child.py [--seed S]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import random
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from device_look_child import default_rooms, look_user, new_room, other_calls  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402

GOLDEN = REPO / "tests" / "golden" / "reference_only" / "rmst.json"
HEAD_TOPICS = b"\n~BB*** Rooms data ***\n\n~FTRoom name            : Access  Users  Mesgs  Topic\n\n"                     # c:5672
HEAD_LINKS = b"\n~BB*** Rooms data ***\n\n~FTRoom name            : Access  Users  Mesgs  Inlink  LStat  Service\n\n"  # c:5673
CAPACITIES = (1, 64, 65, 257, 1025)
LOOK_ROOMS = (1, 2, 64, 65, 1024)
LOOKERS_PER_CALL = 8
COMMANDS = {".rmst": (device.COM_RMST, True), ".rmsn": (device.COM_RMSN, False)}
STATS = {None: b"   -", device.LINK_DOWN: b"~FRDOWN", device.LINK_VERIFYING: b" ~FYVER", device.LINK_UP: b"  ~FGUP"}
USER_FIELDS = ("room", "login", "colour", "name", "vis", "level")
ROOM_FIELDS = ("name", "access", "topic", "mesg_cnt", "netlink", "inlink")


# ------------------------------------------------------------------ the model
def list_room(name=b"room", **fields) -> dict:
    """A room as rooms() reads it: new_room's fields, ``inlink``, and a netlink of ``(service, allow_in, state)``."""
    return new_room(name, **{"inlink": False, **fields})


def link_state(rm: dict):
    """None without a netlink; a 2-tuple is a link that is UP."""
    link = rm["netlink"]
    return None if link is None else link[2] if len(link) == 3 else device.LINK_UP


def counted(users: dict, r: int) -> int:
    """c:5679-5680 over the slots: a slot without a name is no user, and one at login stage has no room yet."""
    return sum(1 for u in users.values() if u["name"] and not u["login"] and u["room"] == r)


def room_line(rm: dict, count: int, topics: bool) -> bytes:
    access = bytearray(b" ~FRPRIV" if rm["access"] & 1 else b"  ~FGPUB")                             # c:5675-5677
    if rm["access"] & 2:
        access[0] = ord("*")
    if topics:
        return b"%-20s : %9s~RS    %3d    %3d  %s\n" % (rm["name"], bytes(access), count, rm["mesg_cnt"], rm["topic"])
    state = link_state(rm)
    stat = STATS[device.LINK_DOWN] if state is None and rm["inlink"] else STATS[state]                # c:5685-5693
    serv = rm["netlink"][0] if rm["netlink"] else b""
    return b"%-20s : %9s~RS    %3d    %3d     %s   %s~RS  %s\n" % (rm["name"], bytes(access), count, rm["mesg_cnt"],
                                                                     b"YES" if rm["inlink"] else b" NO", stat, serv)


def rooms(users: dict, rms, topics: bool) -> list:
    """The strings rooms(user, show_topics) hands to write_user, in order: whoever looks."""
    out = [HEAD_TOPICS if topics else HEAD_LINKS]
    out += [room_line(rm, counted(users, r), topics) for r, rm in enumerate(rms) if rm["name"]]
    return out + [b"\n"]


def model_chunks(users: dict, rms, slot: int, topics: bool) -> list:
    c = int(users[slot]["colour"])
    return [ch for s in rooms(users, rms, topics) for ch in nuts_path.chunks(s, c)]


def seat(roster: device.Roster, u: dict) -> None:
    fields = {f: u[f] for f in USER_FIELDS if f != "name"}
    if u["name"]:
        fields["name"] = u["name"]
    roster.update(u["slot"], **fields)


def set_rooms(roster: device.Roster, rms) -> None:
    ids = list(range(len(rms)))
    roster.set_rooms(ids, **{f: [rms[i][f] for i in ids] for f in ROOM_FIELDS})


# ------------------------------------------------------------------ the recorded session
def session_rooms() -> list:
    """The rooms rmst.json was recorded with: the default ones, the lounge an ACCEPT room (inlink), the corridor with a
    netlink to the service ``faraway`` that is never dialled."""
    rms = [list_room(**{k: v for k, v in rm.items() if k != "name"}, name=rm["name"]) for rm in default_rooms()]
    by_name = {rm["name"]: rm for rm in rms}
    by_name[b"lounge"]["inlink"] = True
    by_name[b"corridor"]["netlink"] = (b"faraway", False, device.LINK_DOWN)
    return rms


def golden_listings() -> int:
    doc = json.loads(GOLDEN.read_text())
    return sum(s.get("send") in COMMANDS for s in doc["steps"])


def replay_listings(answer) -> dict:
    """tests/golden/reference_only/rmst.json: a client gets the next slot as it connects, at the name prompt (``login``
    set, no name, no room); its login seats the account there, in room 0.  A ``.go`` that succeeded moves its actor,
    ``.topic`` and ``.write`` change its room's record, ``.private`` the room's access, ``.invis`` its actor.  The clone
    of ``.clone`` is no slot.  ``answer(users, rms, slot, line)`` must be, byte for byte, what the actor of a listing
    received."""
    doc = json.loads(GOLDEN.read_text())
    accounts = {a["name"]: a for a in doc["accounts"][0]}
    rms = session_rooms()
    seats, users = {}, {}
    res = {"compared": 0, "mismatches": [], "kinds": {}}
    for step in doc["steps"]:
        actor, send = step["actor"], step.get("send", "")
        u = users.get(seats.get(actor))
        if step["op"] == "connect":
            seats[actor] = len(seats)
            users[seats[actor]] = look_user(seats[actor], room=None, login=1, level=0)
        elif step["op"] == "login":
            acc = accounts[step["name"]]
            u.update(room=0, login=0, name=acc["name"].encode("latin-1"), level=int(acc["level"]),
                     colour=int(bool(acc["colour"])))
        elif send.startswith(".go ") and "Access is " in step["recv"].get(actor, ""):
            u["room"] = next(i for i, rm in enumerate(rms) if rm["name"].startswith(send[4:].encode()))
        elif send.startswith(".topic "):
            rms[u["room"]]["topic"] = send[len(".topic "):].encode("latin-1")
        elif send.startswith(".write "):
            rms[u["room"]]["mesg_cnt"] += 1
        elif send == ".private" and "PRIVATE" in step["recv"].get(actor, ""):
            rms[u["room"]]["access"] |= device.PRIVATE
        elif send == ".invis":
            u["vis"] = 0
        elif send in COMMANDS:
            kind = send[1:] + ("_colour" if u["colour"] else "_plain")
            res["compared"] += 1
            res["kinds"][kind] = res["kinds"].get(kind, 0) + 1
            got = answer(users, rms, seats[actor], send)
            if got != step["recv"][actor].encode("latin-1"):
                res["mismatches"].append({"step": step.get("note", send), "actor": actor, "got": got.decode("latin-1"),
                                          "want": step["recv"][actor]})
    return res


# ------------------------------------------------------------------ seeded rosters
WORST_TOPICS = (b"", b"~FR" * 20, b"\n" * 60, b"t" * 60, b"a ~FGgreen~RS topic", b"/~" * 30, b"\xe9\xff high")
WORST_NAMES = (b"n" * 20, b"a", b"~FR~FG~FB~FT~OL~UL~", b"\n" * 20, b"drive")
SERVICES = (b"", b"s" * 80, b"faraway", b"~FR" * 26 + b"~F", b"\n" * 80)


def fuzz_room(rng: random.Random, nameless: bool) -> dict:
    state = rng.choice((None, device.LINK_DOWN, device.LINK_VERIFYING, device.LINK_UP, "old"))
    link = None if state is None else (rng.choice(SERVICES), rng.random() < 0.5) + (() if state == "old" else (state,))
    return list_room(b"" if nameless else rng.choice(WORST_NAMES + (b"R%d" % rng.randrange(10**6),)), access=rng.randrange(4),
                     topic=rng.choice(WORST_TOPICS), mesg_cnt=rng.choice((0, 1, 99, 100, 999, 1000, 2**31 - 1, rng.randrange(2**31))),
                     netlink=link, inlink=rng.random() < 0.5)


def fuzz_roster(rng: random.Random, cap: int, nr: int, fill: str):
    """``cap`` slots over ``nr`` look rooms.  ``fill``: "one" puts every user into one room, "spread" spreads them, so
    that rooms stay empty or hold one user when there are more rooms than slots.  A fifth of the slots are no counted
    user: nameless, at login stage, roomless, or in a room at or past ``nr``.  Every eighth room has no name."""
    rms = [fuzz_room(rng, nameless=nr > 2 and i % 8 == 5) for i in range(nr)]
    roster = device.Roster(cap, look_rooms=nr)
    set_rooms(roster, rms)
    full = rng.randrange(nr)
    users = {}
    for j in range(cap):
        u = look_user(j, name=b"U%d" % j, room=full if fill == "one" else rng.randrange(nr), colour=rng.randrange(2),
                      vis=int(rng.random() < 0.8), level=rng.randrange(5))
        if cap > 4 and rng.random() < 0.2:
            kind = rng.randrange(4)
            if kind == 0:
                u["name"] = None
            elif kind == 1:
                u["login"] = 1
            elif kind == 2:
                u["room"] = None
            else:
                u["room"] = nr + rng.choice((0, 1, 5000, device.ROOM_LIMIT - 1 - nr))
        users[j] = u
    for f in USER_FIELDS:                                   # field by field: 1,025 updates of one slot each are slow
        if f == "name":
            named = [j for j in users if users[j]["name"]]
            roster.update(named, name=[users[j]["name"] for j in named])
        else:
            roster.update(list(users), **{f: [users[j][f] for j in users]})
    return roster, users, rms


def rooms_differences(users: dict, rms, slots, kinds, got: device.Rooms, seen: dict) -> list:
    bad, nr = [], len(rms)
    want_counts = [counted(users, r) for r in range(nr)]
    if got.counts.dtype != np.int32 or got.counts.tolist() != want_counts:
        bad.append({"what": "counts", "device": got.counts.tolist()[:20], "model": want_counts[:20]})
    strings = {device.ROOMS_TAIL: b"\n"}
    for topics, head, first in ((True, device.ROOMS_HEAD_TOPICS, 3), (False, device.ROOMS_HEAD_LINKS, 3 + nr)):
        if topics in kinds:
            strings[head] = HEAD_TOPICS if topics else HEAD_LINKS
            strings.update({first + r: room_line(rm, want_counts[r], topics) for r, rm in enumerate(rms) if rm["name"]})
    if len(got.text_sizes) != 3 + 2 * nr:
        bad.append({"what": "texts", "device": len(got.text_sizes), "model": 3 + 2 * nr})
    for t in range(3 + 2 * nr):
        if t not in strings:                                # a kind not asked for, a nameless room: void, no variants
            if got.text_sizes[t] != -1 or got.variant_sizes[t].tolist() != [0, 0] or got.write_counts[t].tolist() != [0, 0]:
                bad.append({"what": "void", "text": t, "size": int(got.text_sizes[t])})
                break
            continue
        s = strings[t]
        if got.text(t) != s:
            bad.append({"what": "text", "text": t, "device": got.text(t).decode("latin-1"), "model": s.decode("latin-1")})
            break
        for c in (0, 1):
            ch = nuts_path.chunks(s, c)
            if got.text_chunks(t, c) != ch or got.write_sizes[t, c, :got.write_counts[t, c]].tolist() != [len(x) for x in ch]:
                bad.append({"what": "variant", "text": t, "colour": c})
                break
    for k, (slot, topics) in enumerate(zip(slots, kinds)):
        want = model_chunks(users, rms, slot, topics)
        if got.chunks(k) != want or got.output(k) != b"".join(want) or bool(got.topics[k]) != topics:
            bad.append({"what": "chunks", "looker": k, "slot": slot, "topics": topics})
        seen["colours"].add(int(users[slot]["colour"]))
    seen["empty"] += sum(n == 0 for n in want_counts)
    seen["single"] += sum(n == 1 for n in want_counts)
    seen["all"] += sum(n and n == sum(want_counts) for n in want_counts)
    seen["uncounted"] += len(users) - sum(want_counts)
    seen["nameless_rooms"] += sum(not rm["name"] for rm in rms)
    seen["states"] |= {str(link_state(rm)) for rm in rms}
    seen["inlinks"] |= {bool(rm["inlink"]) for rm in rms}
    seen["fixed"] += sum(bool(rm["access"] & 2) for rm in rms)
    return bad


def cases() -> list:
    """(capacity, look rooms, fill, kinds of the 8 lookers): every capacity with every room count at least once, the
    largest with both fills, and calls of one kind only."""
    mixed = (True, False, False, True, True, False, True, False)
    out = []
    for i, cap in enumerate(CAPACITIES):
        for j, nr in enumerate(LOOK_ROOMS):
            kinds = mixed if (i + j) % 3 else ((True,) * 8 if (i + j) % 2 else (False,) * 8)
            out.append((cap, nr, "one" if (i + j) % 4 == 1 else "spread", kinds))
    return out + [(1025, 1024, "one", mixed), (1025, 2, "one", mixed)]


def fuzz_part(seed: int) -> dict:
    rng = random.Random(seed)
    seen = {"colours": set(), "empty": 0, "single": 0, "all": 0, "uncounted": 0, "nameless_rooms": 0, "states": set(),
            "inlinks": set(), "fixed": 0}
    bad, one_kind = [], 0
    for cap, nr, fill, kinds in cases():
        roster, users, rms = fuzz_roster(rng, cap, nr, fill)
        slots = [rng.randrange(cap) for _ in range(LOOKERS_PER_CALL - 1)]
        slots.append(slots[0])                              # duplicates are allowed
        got = roster.rooms_many(slots, topics=list(kinds))
        bad += [{"capacity": cap, "look_rooms": nr, **b} for b in rooms_differences(users, rms, slots, kinds, got, seen)]
        one_kind += len(set(kinds)) == 1
        roster.close()
    return {"capacities": sorted({c[0] for c in cases()}), "look_rooms": sorted({c[1] for c in cases()}), "calls": len(cases()),
            "one_kind_calls": one_kind, "colours": sorted(seen["colours"]), "empty": seen["empty"], "single": seen["single"],
            "all": seen["all"], "uncounted": seen["uncounted"], "nameless_rooms": seen["nameless_rooms"],
            "states": sorted(seen["states"]), "inlinks": sorted(seen["inlinks"]), "fixed": seen["fixed"], "n_bad": len(bad),
            "first_bad": bad[:1]}


def worst_rooms() -> list:
    """The longest lines: a 20-byte name, a fixed private room, a mesg_cnt of 2^31 - 1, a 60-byte topic, inlink, a link that
    is down and an 80-byte service -- of plain bytes, of colour commands, and of newlines, which the transducer widens."""
    link = lambda serv: (serv, True, device.LINK_DOWN)
    return [list_room(b"n" * 20, access=device.FIXED_PRIVATE, topic=b"t" * 60, mesg_cnt=2**31 - 1, netlink=link(b"s" * 80), inlink=True),
            list_room(b"~FR~FG~FB~FT~OL~UL~", access=device.FIXED_PRIVATE, topic=b"~FR" * 20, mesg_cnt=2**31 - 1,
                      netlink=link(b"~FR" * 26 + b"~F"), inlink=True),
            list_room(b"\n" * 20, access=device.PRIVATE, topic=b"\n" * 60, mesg_cnt=2**31 - 1, netlink=link(b"\n" * 80), inlink=True)]


def widening_part() -> dict:
    """65,536 named users in one of two rooms whose mesg_cnt is 2^31 - 1: the counts before and after one slot moves."""
    cap = device.MAX_CAPACITY
    rms = worst_rooms()[:2]
    roster = device.Roster(cap, look_rooms=2)
    set_rooms(roster, rms)
    roster.update(list(range(cap)), room=0, name=[b"U%d" % j for j in range(cap)])
    users = {j: look_user(j, name=b"U%d" % j, room=0) for j in range(cap)}
    out = {}
    for when in ("before", "after"):
        got = roster.rooms_many([0, cap - 1], topics=[True, False])
        want = [counted(users, 0), counted(users, 1)]
        lines = [got.text(3), got.text(4), got.text(5), got.text(6)]
        model = [room_line(rms[r], want[r], t) for t in (True, False) for r in (0, 1)]
        out[when] = {"counts": got.counts.tolist(), "model_counts": want, "lines_match": lines == model,
                     "chunks_match": all(got.chunks(k) == model_chunks(users, rms, s, t) for k, (s, t) in enumerate(((0, True), (cap - 1, False)))),
                     "longest": [len(lines[0]), len(lines[2])]}
        roster.update(40_000, room=1)
        users[40_000]["room"] = 1
    roster.close()
    return out


def longest_part() -> dict:
    rms = worst_rooms()
    roster = device.Roster(2, look_rooms=len(rms))
    set_rooms(roster, rms)
    users = {0: look_user(0, name=b"A", room=0, colour=1), 1: look_user(1, name=b"B", room=1)}
    for u in users.values():
        seat(roster, u)
    got = roster.rooms_many([0, 1], topics=[True, False])
    bad = rooms_differences(users, rms, [0, 1], (True, False), got, {"colours": set(), "empty": 0, "single": 0, "all": 0, "uncounted": 0,
                                                                      "nameless_rooms": 0, "states": set(), "inlinks": set(), "fixed": 0})
    nr = len(rms)
    roster.close()
    return {"n_bad": len(bad), "first_bad": bad[:1],
            "rmst": {"bytes": int(got.variant_sizes[3:3 + nr].max()), "writes": int(got.write_counts[3:3 + nr].max())},
            "rmsn": {"bytes": int(got.variant_sizes[3 + nr:].max()), "writes": int(got.write_counts[3 + nr:].max())}}


def digest(got: device.Rooms) -> str:
    h = hashlib.sha256()
    for k in range(len(got.slots)):
        h.update(b"".join(got.chunks(k)) + bytes([0]) + bytes(len(c) % 251 for c in got.chunks(k)))
    h.update(got.counts.tobytes())
    return h.hexdigest()


def determinism_part(seed: int) -> dict:
    out = []
    for _ in range(2):
        rng = random.Random(seed)
        roster, users, rms = fuzz_roster(rng, 1025, 65, "spread")
        call = lambda: digest(roster.rooms_many([0, 1, 1024, 0], topics=[True, False, True, False]))
        out.append([call(), call()])
        roster.close()
    return {"same_on_a_second_call": out[0][0] == out[0][1], "same_on_a_second_roster": out[0] == out[1]}


def nothing_else_moved_part() -> dict:
    cap = 300
    rms = [list_room(b"R" * 20), list_room(b"twelve_bytes", inlink=True), list_room(b"e", netlink=(b"in", True, device.LINK_VERIFYING)),
           list_room(b"far", netlink=(b"s" * 80, False))]

    def build(clones=0):
        r = device.Roster(cap, review_rooms=2, look_rooms=len(rms), clones=clones)
        r.update(list(range(cap)), room=[j % 2 for j in range(cap)], colour=[j % 3 == 0 for j in range(cap)],
                 name=[b"U%d" % j for j in range(cap)], level=2)
        r.update([0, 1], name=[b"Alice", b"Bobby"])
        set_rooms(r, rms)
        if clones:
            r.set_clones(0, owner=0, room=1, hear=device.CLONE_HEAR_ALL)
        return r

    def relay(r):
        """relay_many needs clone records, which plan_many of other_calls refuses: a pair of rosters of its own."""
        rl = r.relay_many([(b"hi ~FRthere~RS\n", 1, 1, 0, 3)])
        return [rl.relay_bits.tolist(), rl.relay_text(0).hex(), [c.hex() for c in rl.relay_chunks(0, 1)], rl.timing["h2d_bytes"]]

    def listed(r):
        """The calls other_calls does not make."""
        lk, w = r.look_many([0, 1]), r.who_many([0, 1], now=77, date=b"DATE")
        return {"look": [lk.output(0).hex(), lk.output(1).hex(), lk.timing["h2d_bytes"]],
                "who": [w.output(0).hex(), w.output(1).hex(), w.timing["h2d_bytes"]]}

    fresh, asked = build(), build()
    out = {"capacity": cap, "look_rooms": len(rms), "fresh": other_calls(fresh), "before_rooms": other_calls(asked)}
    h = {}
    call = lambda: asked.rooms_many([0, 1, 2], topics=[True, False, True]).timing["h2d_bytes"]
    h["first"] = call()
    h["clean"] = [call() for _ in range(2)]
    for r in (asked, fresh):                                # the same updates to both: the other calls must answer alike
        r.set_rooms(1, topic=b"new topic")
    h["after_set_rooms"] = call()
    for r in (asked, fresh):
        r.update(7, desc=b"changed", last_login=5, afk_mesg=b"brb")
    h["after_updates_of_others"] = call()
    h["clean_again"] = call()
    out["rooms_h2d"] = h
    out["listed_after_rooms"], out["listed_fresh"] = listed(asked), listed(fresh)
    out["after_rooms"] = other_calls(asked)                 # and the other calls still answer alike
    out["fresh_again"] = other_calls(fresh)
    users = {j: look_user(j, name=b"U%d" % j, room=j % 2, colour=int(j % 3 == 0), level=2) for j in range(cap)}
    rms[1]["topic"] = b"new topic"
    got = asked.rooms_many([0, 1], topics=[True, False])
    out["still_right"] = all(got.chunks(k) == model_chunks(users, rms, k, t) for k, t in ((0, True), (1, False)))
    fresh.close()
    asked.close()
    fresh, asked = build(clones=2), build(clones=2)
    asked.rooms_many([0, 1], topics=True)
    asked.rooms_many([0], topics=False)
    out["relay_after_rooms"], out["relay_fresh"] = relay(asked), relay(fresh)
    fresh.close()
    asked.close()
    return out


def regrown_part() -> dict:
    """A roster whose device allocation was freed and made anew by a larger call between two rooms_many calls: the second
    finds the table gone from the device and must still count right.  Paired with a roster that saw no such call."""
    cap, nr = 65, 1024
    rng = random.Random(11)
    rms = [fuzz_room(rng, nameless=i % 8 == 5) for i in range(nr)]
    users = {j: look_user(j, name=b"U%d" % j, room=(37 * j) % 70, colour=j % 2) for j in range(cap)}

    def build():
        r = device.Roster(cap, look_rooms=nr)
        set_rooms(r, rms)
        r.update(list(range(cap)), room=[users[j]["room"] for j in range(cap)], colour=[j % 2 for j in range(cap)],
                 name=[b"U%d" % j for j in range(cap)])
        return r

    right = lambda g: all(g.chunks(k) == model_chunks(users, rms, k, t) for k, t in ((0, True), (1, False)))
    grown, plain = build(), build()
    # a tiny call uploads the table and the speaker state; the rooms call after it needs 4 MB, so it finds the allocation
    # freed and made anew, and must upload the table from the pinned mirror though the roster passes it the room table alone
    grown.speak_many([(0, device.COM_SAY, b"hi", 1)])
    passed_clean = not grown._dirty and not grown._speech_dirty and grown._rooms_dirty
    first = [r.rooms_many([0, 1], topics=[True, False]) for r in (grown, plain)]
    out = {"passed_the_room_table_alone": passed_clean, "first_alike": digest(first[0]) == digest(first[1]), "first_right": right(first[0]),
           "first_h2d": [int(g.timing["h2d_bytes"]) for g in first]}
    # and the other way round: a far larger call of another kind regrows it between two rooms calls
    grown.plan_many([(b"x" * 1900 + b"\n", None, None, 0, 3)] * 400)      # 9 MB of variants in the roster's allocation
    for r in (grown, plain):
        r.update(5, room=3)
    users[5]["room"] = 3
    second = [r.rooms_many([0, 1], topics=[True, False]) for r in (grown, plain)]
    out.update({"second_alike": digest(second[0]) == digest(second[1]), "second_right": right(second[0]),
                "counted": int(second[0].counts.sum()), "model_counted": sum(counted(users, r) for r in range(nr))})
    grown.close()
    plain.close()
    return out


def golden_part() -> dict:
    rms = session_rooms()
    roster = device.Roster(8, look_rooms=len(rms))
    vs_model, dispatched = [], []

    def answer(users, rms_, slot, line):
        set_rooms(roster, rms_)
        for u in users.values():
            seat(roster, u)
        inp = roster.input_many([(slot, line.encode() + b"\n")])
        dispatched.append([int(inp.kind[0]), int(inp.com[0])])
        com, topics = COMMANDS[line]
        if dispatched[-1] != [device.COMMAND, com]:
            return b"not dispatched as command %d" % com
        got = roster.rooms_many([slot], topics=topics)
        if got.chunks(0) != model_chunks(users, rms_, slot, topics):
            vs_model.append(slot)
        return got.output(0)

    res = replay_listings(answer)
    roster.close()
    return {"compared": res["compared"], "mismatches": res["mismatches"][:2], "n_bad_vs_model": len(vs_model), "kinds": res["kinds"],
            "dispatched": sorted({tuple(d) for d in dispatched})}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20262)
    args = ap.parse_args()
    if device.device_count() < 1:
        print("no GPU visible", file=sys.stderr)
        return 3
    res = {"golden": golden_part(), "fuzz": fuzz_part(args.seed), "longest": longest_part(), "widening": widening_part(),
           "determinism": determinism_part(args.seed + 2), "moved": nothing_else_moved_part(), "regrown": regrown_part()}
    print("DEVICE_ROOMS " + json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
