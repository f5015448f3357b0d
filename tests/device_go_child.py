"""The device work of tests/test_device_go.py, in a short-lived child process of its own, and the CPU model the host tier
of that module shares with it.

As tests/device_rooms_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_GO {...}``).  ``go`` is the Python model of ``go()``, ``move_user()`` and what ``reset_access()``
decides (nuts333.c:4305-4459, 2087-2106), built from the reference's format strings; ``go_call`` is the model of one
``Roster.go_many`` call: it runs the events ONE AFTER ANOTHER, each against the state the earlier ones left, and defers by
the rule of the call -- so a device that decides every event against the snapshot agrees with it only if the rule makes
the two the same.  ``GoReplayer`` answers the ``.go`` steps of the recorded sessions through a backend's ``go`` method and
compares every client's bytes, the mover's included.

    python tests/device_go_child.py [--seed S]
"""
from __future__ import annotations

import random
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import session_replay as sr  # noqa: E402
from device_look_child import look_user  # noqa: E402
from device_look_child import model_chunks as look_chunks  # noqa: E402
from device_rooms_child import counted, list_room  # noqa: E402
from event_checks import child_main, event_differences, lines_of, load, plan_of  # noqa: E402
from event_checks import digest as digest_of  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402

SESSIONS = ("reference_only/go.json", "rooms.json", "reference_only/rmst.json", "reference_only/who.json", "clones.json") + tuple(
    f"reference_only/replay_{seed}.json" for seed in sr.FIRST_SEEDS)
WIZ, ARCH = 2, 3
MOVED = (device.GO_WALKED, device.GO_TELEPORTED, device.GO_UNSEEN)
GO_WHERE, NOSUCHROOM = b"Go where?\n", b"There is no such room.\n"                       # c:4313, nuts333.h:145
PRIVATE_ROOM = b"That room is currently private, you cannot enter.\n"                    # c:4418
INVISENTER, INVISLEAVE = b"A presence enters the room...\n", b"A presence leaves the room.\n"   # nuts333.h:148-149
RESET_LINE = b"Room access returned to ~FGPUBLIC.\n"                                     # c:2097
CAPACITIES = (1, 63, 64, 65, 256, 257)
LOOK_ROOMS = (1, 6, 255, 256, 257)
EVENTS = (1, 2, 64, 65)
USER_FIELDS = ("room", "login", "colour", "ignall", "name", "vis", "level", "afk", "desc")
WORST_PHRASES = (b"", b"p" * 40, b"~FR" * 13 + b"~", b"\n" * 40, b"slides in", b"/~" * 20, b"\xe9\xff high")


# ------------------------------------------------------------------ the model
def go_user(slot: int, **fields) -> dict:
    return look_user(slot, **{"in_phrase": b"enters", "out_phrase": b"goes", "invite": None, "ignshout": 0, **fields})


def first_word(inpstr: bytes) -> bytes:
    """word[1] of the reference: the first word of inpstr as wordfind() finds it, cut at 39 bytes."""
    words = sr.words_of(inpstr)
    return words[0] if words else b""


def get_room(rooms, word: bytes):
    """c:2388-2389 over rooms that have a name: the first whose name begins with the word."""
    return next((i for i, r in enumerate(rooms) if r["name"] and r["name"].startswith(word)), None)


def has_room_access(u: dict, rooms, rm: int, gatecrash: int) -> bool:
    access = rooms[rm]["access"]                                        # c:2416-2420
    return not (access & device.PRIVATE and u["level"] < gatecrash and u["invite"] != rm
                and not (access & 2 and u["level"] >= WIZ))


def population(users: dict, clones, rm: int, but: int) -> int:
    """Who reset_access counts in rm once ``but`` has left (c:2095): the users with a name and no login flag, and the clones."""
    return (sum(1 for j, u in users.items() if j != but and u["room"] == rm and u["name"] and not u["login"])
            + sum(1 for c in clones if c is not None and c[1] == rm))


def go(users: dict, rooms, clones, slot: int, inpstr: bytes, wc: int, gatecrash: int, min_private: int) -> dict:
    """What one ``.go`` does, without doing it: the outcome, the room the word resolved to, and the four texts."""
    u = users[slot]
    here = u["room"]
    res = {"slot": slot, "outcome": None, "target": -1, "old": here, "returned": False, "enter": None, "leave": None,
           "reset": None, "reply": None}
    word = first_word(inpstr)
    if wc < 2:
        res.update(outcome=device.GO_WHERE, reply=GO_WHERE)
        return res
    if rooms[here]["netlink"] is not None and rooms[here]["netlink"][0].startswith(word):         # c:4315-4316
        res["outcome"] = device.GO_NETLINK
        return res
    rm = get_room(rooms, word)
    if rm is None:
        res.update(outcome=device.GO_NO_ROOM, reply=NOSUCHROOM)
        return res
    res["target"] = rm
    name, linked = rooms[rm]["name"], rm in rooms[here]["links"]
    if rm == here:
        res.update(outcome=device.GO_ALREADY, reply=b"You are already in the %s!\n" % name)
    elif not linked and u["level"] < WIZ:
        res.update(outcome=device.GO_NOT_ADJOINED, reply=b"The %s is not adjoined to here.\n" % name)
    elif not has_room_access(u, rooms, rm, gatecrash):
        res.update(outcome=device.GO_PRIVATE, reply=PRIVATE_ROOM)
    else:
        me = u["name"]
        if not u["vis"]:
            res.update(outcome=device.GO_UNSEEN, enter=INVISENTER, leave=INVISLEAVE)
        elif not linked:
            res.update(outcome=device.GO_TELEPORTED, enter=b"~FT~OL%s appears in an explosion of blue magic!\n" % me,
                       leave=b"~FT~OL%s chants a spell and vanishes into a magical blue vortex!\n" % me)
        else:
            res.update(outcome=device.GO_WALKED, enter=b"%s %s.\n" % (me, u["in_phrase"]),
                       leave=b"%s %s to the %s.\n" % (me, u["out_phrase"], name))
        if rooms[here]["access"] == device.PRIVATE and population(users, clones, here, slot) < min_private:
            res.update(returned=True, reset=RESET_LINE)
    return res


def admitted(users: dict, rm: int, sender) -> list:
    """write_room_except(rm, text, sender) over the slots (c:1410-1415); com_num is GO, so ignshout plays no part."""
    return [j for j, u in sorted(users.items())
            if u["room"] == rm and not u["login"] and not u["ignall"] and j != sender]


def look_of(users: dict, rooms, slot: int) -> list:
    """look()'s chunks for users[slot]: it shows a netlink only when the link is UP (c:3966)."""
    seen = [rm if rm["netlink"] is None or len(rm["netlink"]) < 3 or rm["netlink"][2] == device.LINK_UP else {**rm, "netlink": None}
            for rm in rooms]
    return look_chunks(users, seen, slot)


def apply_move(users: dict, rooms, res: dict, cleared: list) -> None:
    """move_user's and reset_access's changes of state (c:4422, 4456, 2098-2104); between the two it looks (c:4457), and
    the look's chunks are kept in ``res``."""
    u = users[res["slot"]]
    if u["invite"] == res["target"]:
        u["invite"] = None
    u["room"] = res["target"]
    if "look" not in res and users[res["slot"]].get("name"):
        res["look"] = look_of(users, rooms, res["slot"])
    if res["returned"]:
        rooms[res["old"]]["access"] = device.PUBLIC
        for x in users.values():
            if x["invite"] == res["old"]:
                x["invite"] = None
        cleared.append(res["old"])


def go_call(users: dict, rooms, clones, events, gatecrash: int, min_private: int) -> dict:
    """One go_many call: the events one after another on ``users`` and ``rooms``, which it changes.  Returns the events'
    results -- a deferred one has the outcome GO_DEFERRED and no text -- with the plans of their texts, the rooms whose
    review ring was cleared, and the movers in event order."""
    touched_slots, touched_rooms, out, cleared, movers = set(), set(), [], [], []
    for slot, inpstr, wc in events:
        res = go(users, rooms, clones, slot, inpstr, wc, gatecrash, min_private)
        # the call's rule, and the binding's: a move next to a room that an earlier event returned to public
        if (slot in touched_slots or res["old"] in touched_rooms or res["target"] in touched_rooms
                or (res["outcome"] in MOVED and set(cleared) & set(rooms[res["target"]]["links"]))):
            res.update(outcome=device.GO_DEFERRED, returned=False, enter=None, leave=None, reset=None, reply=None)
        res["plans"] = {"enter": admitted(users, res["target"], None) if res["enter"] is not None else [],
                        "leave": admitted(users, res["old"], slot) if res["leave"] is not None else [],
                        "reset": admitted(users, res["old"], slot) if res["reset"] is not None else [],
                        "reply": [slot] if res["reply"] is not None else []}
        if res["outcome"] in MOVED:
            touched_slots.add(slot)
            touched_rooms |= {res["old"], res["target"]}
            apply_move(users, rooms, res, cleared)
            movers.append(slot)
        out.append(res)
    return {"events": out, "cleared": cleared, "movers": movers}


def deliveries(users: dict, rooms, call: dict) -> dict:
    """What every slot receives of a go_call, after it: per event the enter line, the leave line, the mover's look, the
    reset line, or the reply; the moves are all applied, and a look shows the state after ALL of them only when the
    call had one mover -- the replayer's calls have one event."""
    out = {j: b"" for j in users}
    for res in call["events"]:
        for kind in ("enter", "leave"):
            for j in res["plans"][kind]:
                out[j] += b"".join(nuts_path.chunks(res[kind], users[j]["colour"]))
        if res["outcome"] in MOVED:
            out[res["slot"]] += b"".join(res["look"])
        for kind in ("reset", "reply"):
            for j in res["plans"][kind]:
                out[j] += b"".join(nuts_path.chunks(res[kind], users[j]["colour"]))
    return out


# ------------------------------------------------------------------ a roster and its model
ROOM_FIELDS = ("name", "access", "desc", "links", "topic", "mesg_cnt", "netlink", "inlink")


def set_rooms(roster: device.Roster, rooms) -> None:
    ids = list(range(len(rooms)))
    roster.set_rooms(ids, **{f: [rooms[i][f] for i in ids] for f in ROOM_FIELDS})


def seat(roster: device.Roster, users: dict, slots=None) -> None:
    """The users' fields into the roster, field by field."""
    ids = sorted(users) if slots is None else list(slots)
    if not ids:
        return
    for f in USER_FIELDS:
        if f == "name":
            named = [j for j in ids if users[j]["name"]]
            if named:
                roster.update(named, name=[users[j]["name"] for j in named])
        elif f == "afk":
            roster.update(ids, afk=[int(bool(users[j]["afk"])) for j in ids])
        else:
            roster.update(ids, **{f: [users[j][f] for j in ids]})
    roster.update(ids, in_phrase=[users[j]["in_phrase"] for j in ids], out_phrase=[users[j]["out_phrase"] for j in ids],
                  invite_room=[users[j]["invite"] for j in ids])


def seat_clones(roster: device.Roster, clones) -> None:
    for c, rec in enumerate(clones):
        if rec is None:
            roster.set_clones(c, owner=None)
        else:
            roster.set_clones(c, owner=rec[0], room=rec[1], hear=rec[2])


def texts_of(got: device.Go):
    return (("enter", got.enter, got.enter_text), ("leave", got.leave, got.leave_text), ("reset", got.reset, got.reset_text),
            ("reply", got.reply, got.reply_text))


def go_differences(got: device.Go, call: dict, users: dict, rooms) -> list:
    """Everything a Go says against the model's call; ``users`` and ``rooms`` are the state after it."""
    bad = event_differences(
        got, call, texts_of(got), device.GO_DEFERRED,
        lambda k, res: ((int(got.target[k]), int(got.old_room[k]), bool(got.returned_public[k])), (res["target"], res["old"], res["returned"])),
        also_deferred=lambda k: got.returned_public[k])
    movers = call["movers"]
    if (got.look is None) != (not movers) or got.moved().tolist() != [k for k, r in enumerate(call["events"]) if r["outcome"] in MOVED]:
        bad.append({"what": "movers", "device": got.moved().tolist()})
    elif movers:
        if got.look.slots.tolist() != movers or got.look_index[got.moved()].tolist() != list(range(len(movers))):
            bad.append({"what": "look slots", "device": got.look.slots.tolist(), "want": movers})
        else:
            looks = [r["look"] for r in call["events"] if r["outcome"] in MOVED]
            for i, slot in enumerate(movers):
                if got.look.chunks(i) != looks[i]:
                    bad.append({"what": "look", "slot": slot, "room": users[slot]["room"]})
    return bad


def mirror_differences(roster: device.Roster, users: dict, rooms) -> list:
    bad = []
    for j, u in users.items():
        if int(roster._room[j]) != (-1 if u["room"] is None else u["room"]):
            bad.append({"what": "room mirror", "slot": j, "device": int(roster._room[j]), "want": u["room"]})
        if int(roster._go_invite[j]) != (-1 if u["invite"] is None else u["invite"]):
            bad.append({"what": "invite mirror", "slot": j, "device": int(roster._go_invite[j]), "want": u["invite"]})
    for r, rm in enumerate(rooms):
        if int(roster._room_rec[r, 21]) != rm["access"]:
            bad.append({"what": "access mirror", "room": r, "device": int(roster._room_rec[r, 21]), "want": rm["access"]})
    return bad


def following_differences(roster: device.Roster, users: dict, rooms, rng: random.Random) -> list:
    """A plan_many, a look_many and a rooms_many after the call: they see the moves only if the mirrors went up again."""
    bad = []
    named = [r for r, rm in enumerate(rooms) if rm["name"]]
    rm = rng.choice(named) if named else 0
    plan = roster.plan_many([(b"after the ~FRmoves~RS\n", rm, None, 0, device.COM_SAY)])
    if np.flatnonzero(plan.admitted(0)).tolist() != admitted(users, rm, None):
        bad.append({"what": "plan_many after", "room": rm})
    lookers = [j for j, u in users.items() if u["room"] is not None and u["room"] < len(rooms)][:8]
    if lookers:
        lk = roster.look_many(lookers)
        for i, j in enumerate(lookers):
            if lk.chunks(i) != look_of(users, rooms, j):
                bad.append({"what": "look_many after", "slot": j})
    listing = roster.rooms_many([0], topics=True)
    if listing.counts.tolist() != [counted(users, r) for r in range(len(rooms))]:
        bad.append({"what": "rooms_many after", "device": listing.counts.tolist()[:10]})
    return bad


# ------------------------------------------------------------------ seeded streams
def fuzz_rooms(rng: random.Random, nr: int) -> list:
    """``nr`` rooms whose names are prefixes of one another in no order (``r1`` before or after ``r10``), every eighth one
    without a name, a third private, some with a netlink whose service looks like a room."""
    names = [b"r%d" % i for i in range(nr)]
    rng.shuffle(names)
    rooms = []
    for i in range(nr):
        links = rng.sample(range(nr), min(nr, rng.randrange(0, device.MAX_LINKS + 1)))
        link = None
        if rng.random() < 0.15:
            link = (rng.choice((b"r%d" % rng.randrange(nr), b"faraway", b"s" * 80)), rng.random() < 0.5,
                    rng.choice((device.LINK_DOWN, device.LINK_VERIFYING, device.LINK_UP)))
        rooms.append(list_room(b"" if nr > 2 and i % 8 == 5 else names[i], access=rng.choice((0, 0, 0, 1, 1, 2, 3)), links=links,
                               netlink=link, topic=rng.choice((b"", b"a ~FGtopic")), mesg_cnt=rng.randrange(3)))
    return rooms


def fuzz_users(rng: random.Random, cap: int, nr: int) -> dict:
    users = {}
    crowd = max(1, min(nr, 6))                                          # the rooms most users stand in, so that rooms collide
    for j in range(cap):
        u = go_user(j, name=b"U%d" % j, room=rng.randrange(crowd) if rng.random() < 0.8 else rng.randrange(nr),
                    colour=rng.randrange(2), vis=int(rng.random() < 0.85), level=rng.randrange(5), ignall=int(rng.random() < 0.1),
                    in_phrase=rng.choice(WORST_PHRASES + (b"enters",) * 4), out_phrase=rng.choice(WORST_PHRASES + (b"goes",) * 4),
                    invite=rng.randrange(nr) if rng.random() < 0.3 else None)
        if cap > 4 and rng.random() < 0.15:
            kind = rng.randrange(4)
            if kind == 0:
                u["name"] = None
            elif kind == 1:
                u["login"] = 1
            elif kind == 2:
                u["room"] = None
            else:
                u["room"] = nr + rng.choice((0, 1, 5000))
        users[j] = u
    return users


def movers_of(users: dict, nr: int) -> list:
    return [j for j, u in users.items() if u["name"] and not u["login"] and u["room"] is not None and u["room"] < nr]


def fuzz_events(rng: random.Random, users: dict, rooms, k: int) -> list:
    able = movers_of(users, len(rooms))
    named = [rm["name"] for rm in rooms if rm["name"]] or [b"none"]
    events = []
    for _ in range(k):
        slot = rng.choice(able)
        here = rooms[users[slot]["room"]]
        linked = [rooms[l]["name"] for l in here["links"] if rooms[l]["name"]]
        kind = rng.random()
        if kind < 0.45 and linked:
            word = rng.choice(linked)
        elif kind < 0.7:
            word = rng.choice(named)
        elif kind < 0.8:
            word = rng.choice(named)[:rng.randrange(1, 3)]
        elif kind < 0.85:
            word = rng.choice(named) + b"x"
        elif kind < 0.9 and here["netlink"]:
            word = here["netlink"][0][:rng.randrange(1, 40)]
        elif kind < 0.95:
            word = b"w" * rng.choice((39, 45))
        else:
            word = b""
        inpstr = rng.choice((b"", b" ", b"  ")) + word + rng.choice((b"", b"", b" now", b" \x01"))
        events.append((slot, inpstr, 1 if not word else rng.choice((2, 2, 2, 3, 1))))
    return events


def cases() -> list:
    caps, nrs = list(CAPACITIES), list(LOOK_ROOMS)
    return [(caps[i % len(caps)], nrs[i % len(nrs)]) for i in range(max(len(caps), len(nrs)) + 1)]


def fuzz_part(seed: int) -> dict:
    rng = random.Random(seed)
    bad, outcomes, calls, returned, events_n = [], {}, 0, 0, 0
    for cap, nr in cases():
        rooms, users = fuzz_rooms(rng, nr), fuzz_users(rng, cap, nr)
        if not movers_of(users, nr):
            users[0].update(name=b"U0", login=0, room=0)
        clones = [(rng.randrange(cap), rng.randrange(nr), 2) if rng.random() < 0.5 else None for _ in range(3)]
        roster = device.Roster(cap, look_rooms=nr, clones=len(clones), review_rooms=min(nr, 4))
        set_rooms(roster, rooms)
        seat(roster, users)
        seat_clones(roster, clones)
        for k in EVENTS:
            events = fuzz_events(rng, users, rooms, k)
            gatecrash, min_private = rng.randrange(device.MAX_LEVEL + 1), rng.randrange(4)
            call = go_call(users, rooms, clones, events, gatecrash, min_private)
            got = roster.go_many(events, gatecrash_level=gatecrash, min_private_users=min_private)
            found = go_differences(got, call, users, rooms) + mirror_differences(roster, users, rooms)
            found += following_differences(roster, users, rooms, rng)
            bad += [{"cap": cap, "look_rooms": nr, "k": k, **b} for b in found]
            calls += 1
            events_n += k
            returned += sum(r["returned"] for r in call["events"])
            for r in call["events"]:
                outcomes[r["outcome"]] = outcomes.get(r["outcome"], 0) + 1
        roster.close()
    return {"cases": [list(c) for c in cases()], "events_per_call": list(EVENTS), "calls": calls, "events": events_n,
            "outcomes": {str(k): v for k, v in sorted(outcomes.items())}, "returned_public": returned, "n_bad": len(bad),
            "first_bad": bad[:2]}


# ------------------------------------------------------------------ get_room and population edges
def get_room_part() -> dict:
    out, bad = {}, []
    for label, nr, twins in (("255_256", 300, (255, 256)), ("0_1023", 1024, (0, 1023))):
        rooms = [list_room(b"n%d" % i, links=[]) for i in range(nr)]
        rooms[twins[0]]["name"], rooms[twins[1]]["name"] = b"twinroom_a", b"twinroom_b"
        rooms[3]["name"] = b"exactly_twenty_bytes"
        rooms[7]["name"] = b""                                          # a nameless room in between
        users = {0: go_user(0, name=b"Wiz", room=5, level=WIZ)}
        roster = device.Roster(2, look_rooms=nr)
        set_rooms(roster, rooms)
        seat(roster, users)
        words = (b"twin", b"twinroom_b", b"twinroom_", b"exactly_twenty_bytes", b"exactly_twenty_bytesx", b"exactly_twenty_byte",
                 b"n7", b"n%d" % (nr - 1), b"twinroom_c")
        got_targets = []
        for w in words:                                                 # one event a call: every one is decided afresh
            users[0]["room"] = 5
            roster.update(0, room=5)
            call = go_call(users, rooms, [], [(0, w, 2)], ARCH, 2)
            got = roster.go_many([(0, w, 2)], gatecrash_level=ARCH, min_private_users=2)
            got_targets.append(int(got.target[0]))
            bad += [{"part": label, "word": w.decode(), **b} for b in go_differences(got, call, users, rooms)]
        out[label] = got_targets
        roster.close()
    return {"targets": out, "n_bad": len(bad), "first_bad": bad[:2]}


POPULATION_SLOTS = (0, 63, 64, 255, 256)


def population_part() -> dict:
    """A private room left with exactly min_private_users occupants behind, and with one fewer: the occupants at the
    edges of every lane, ballot word and block, and one clone record; login and nameless slots of the room are not counted."""
    out, bad = {}, []
    rooms0 = [list_room(b"den", access=device.PRIVATE, links=[1]), list_room(b"hall", links=[0])]
    for label, min_private in (("stays_private", 6), ("returns_public", 7)):
        rooms = [dict(r) for r in rooms0]
        users = {j: go_user(j, name=b"U%d" % j, room=0, colour=j % 2) for j in POPULATION_SLOTS}
        users[100] = go_user(100, name=b"Mover", room=0)
        users[1] = go_user(1, name=b"Prompt", room=0, login=1)
        users[2] = go_user(2, name=None, room=0)
        users[3] = go_user(3, name=b"Guest", room=1, invite=0)
        clones = [None, (0, 0, device.CLONE_HEAR_ALL), (0, 1, device.CLONE_HEAR_ALL)]
        roster = device.Roster(257, look_rooms=2, clones=3, review_rooms=2)
        set_rooms(roster, rooms)
        seat(roster, users)
        seat_clones(roster, clones)
        roster.plan_many([(b"kept in the ring\n", 0, None, 0, device.COM_SAY)], record=True)
        events = [(100, b"hall", 2)]
        call = go_call(users, rooms, clones, events, ARCH, min_private)
        got = roster.go_many(events, gatecrash_level=ARCH, min_private_users=min_private)
        bad += [{"part": label, **b} for b in go_differences(got, call, users, rooms) + mirror_differences(roster, users, rooms)]
        out[label] = {"returned": bool(got.returned_public[0]), "behind": population(users, clones, 0, 100),
                      "reset_to": np.flatnonzero(got.reset.admitted(0)).tolist(), "access": int(roster._room_rec[0, 21]),
                      "guest_invite": int(roster._go_invite[3]), "ring_lines": int(roster.review_many([0]).line_counts[0])}
        roster.close()
    return {**out, "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ repeatability, regrowth, limits
def digest(got: device.Go) -> str:
    looks = [got.look.output(i) for i in range(len(got.look.slots))] if got.look is not None else []
    return digest_of(got, [got.target, got.old_room, got.returned_public, *looks], texts_of(got))


def determinism_part(seed: int) -> dict:
    runs = []
    for _ in range(2):
        rng = random.Random(seed)
        rooms, users = fuzz_rooms(rng, 6), fuzz_users(rng, 257, 6)
        roster = device.Roster(257, look_rooms=6)
        set_rooms(roster, rooms)
        seat(roster, users)
        events = fuzz_events(rng, users, rooms, 64)
        first = digest(roster.go_many(events, gatecrash_level=ARCH, min_private_users=2))
        seat(roster, users)                                             # back to where the movers stood
        set_rooms(roster, rooms)
        runs.append([first, digest(roster.go_many(events, gatecrash_level=ARCH, min_private_users=2))])
        roster.close()
    return {"same_on_a_second_call": runs[0][0] == runs[0][1], "same_on_a_second_roster": runs[0] == runs[1]}


def regrown_part(seed: int) -> dict:
    """A small call that moves nobody, then one large enough to make the roster's device allocation grow: the table is
    not dirty, and has to travel again from the pinned mirror."""
    rng = random.Random(seed)
    cap, nr = 65, 6
    rooms, users = fuzz_rooms(rng, nr), fuzz_users(rng, cap, nr)
    roster = device.Roster(cap, look_rooms=nr)
    set_rooms(roster, rooms)
    seat(roster, users)
    mover = movers_of(users, nr)[0]
    small = roster.go_many([(mover, b"", 1)], gatecrash_level=ARCH, min_private_users=2)
    clean = not (roster._dirty or roster._go_dirty or roster._rooms_dirty or roster._speech_dirty)
    events = fuzz_events(rng, users, rooms, 600)
    call = go_call(users, rooms, [], events, ARCH, 2)
    big = roster.go_many(events, gatecrash_level=ARCH, min_private_users=2)
    bad = go_differences(big, call, users, rooms) + mirror_differences(roster, users, rooms)
    bad += following_differences(roster, users, rooms, rng)
    roster.close()
    return {"small_outcome": int(small.outcome[0]), "clean_before": clean, "small_h2d": small.timing["h2d_bytes"],
            "big_h2d": big.timing["h2d_bytes"], "capacity": cap, "events": len(events), "n_bad": len(bad), "first_bad": bad[:2]}


def limits_part() -> dict:
    """65,536 slots, 1,024 look rooms, 65,536 clone records, K = 64: against a model on arrays."""
    cap, nr, k = device.MAX_CAPACITY, device.MAX_LOOK_ROOMS, 64
    rng = np.random.default_rng(7)
    private = set(range(0, 16, 2))
    rooms = [list_room(b"room%04d" % i, links=[(i + 1) % nr], access=device.PRIVATE if i in private else device.PUBLIC) for i in range(nr)]
    room = rng.integers(0, nr, cap).astype(np.int32)
    room[:16] = 2 * (np.arange(16) // 2)                                # two users in each of the private rooms 0, 2 .. 14,
    room[16:] = np.maximum(room[16:], 16)                               # and nobody else below room 16
    roster = device.Roster(cap, look_rooms=nr, clones=device.MAX_CAPACITY)
    set_rooms(roster, rooms)
    ids = list(range(cap))
    roster.update(ids, room=room.tolist(), name=[b"U%d" % j for j in ids], level=1, colour=[j & 1 for j in ids])
    crooms = np.full(device.MAX_CAPACITY, 9, dtype=np.int32)
    crooms[-1] = 6                                                      # the last record stands in private room 6
    roster.set_clones(list(range(device.MAX_CAPACITY)), owner=20, room=crooms.tolist())
    # movers: one of each private pair, then users from the far end of the table
    movers = [2 * i for i in range(8)] + [cap - 1 - i for i in range(k - 8)]
    events = [(j, b"room%04d" % ((int(room[j]) + 1) % nr), 2) for j in movers]
    t0 = time.perf_counter()
    got = roster.go_many(events, gatecrash_level=ARCH, min_private_users=2)
    seconds = time.perf_counter() - t0
    bad, touched_rooms, returned_rooms, want_room = [], set(), set(), room.copy()
    for i, j in enumerate(movers):
        old, new = int(room[j]), (int(room[j]) + 1) % nr
        private_target = new in private
        deferred = old in touched_rooms or new in touched_rooms or (not private_target and (new + 1) % nr in returned_rooms)
        if deferred:
            want = (device.GO_DEFERRED, new, old, False)
        elif private_target:
            want = (device.GO_PRIVATE, new, old, False)
        else:
            # the pair's other user stays behind, and in room 6 the last clone record too
            want = (device.GO_WALKED, new, old, old in private and old != 6)
            touched_rooms |= {old, new}
            returned_rooms |= {old} if want[3] else set()
            want_room[j] = new
        have = (int(got.outcome[i]), int(got.target[i]), int(got.old_room[i]), bool(got.returned_public[i]))
        if have != want:
            bad.append({"event": i, "slot": j, "device": list(have), "want": list(want)})
        elif want[0] == device.GO_WALKED:
            enter = np.flatnonzero(got.enter.admitted(i)).tolist()
            leave = np.flatnonzero(got.leave.admitted(i)).tolist()
            if enter != np.flatnonzero(room == new).tolist() or leave != [x for x in np.flatnonzero(room == old).tolist() if x != j]:
                bad.append({"event": i, "what": "plans"})
            if got.leave_text(i) != b"U%d goes to the room%04d.\n" % (j, new) or got.enter_text(i) != b"U%d enters.\n" % j:
                bad.append({"event": i, "what": "texts", "leave": got.leave_text(i).decode()})
    mirror_ok = bool((roster._room == want_room).all())
    publics = [r for r in sorted(private) if int(roster._room_rec[r, 21]) == device.PUBLIC]
    looks = 0 if got.look is None else len(got.look.slots)
    roster.close()
    return {"capacity": cap, "look_rooms": nr, "clones": device.MAX_CAPACITY, "k": k, "seconds": round(seconds, 3),
            "outcomes": sorted(set(got.outcome.tolist())), "mirror_ok": mirror_ok, "publics": publics, "looks": looks,
            "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ the recorded sessions
INVITE_LINE = "You invite "                                             # nuts333.c: invite()


class GoState(sr.State):
    """The replayer's state with what .go reads: every user's invite, the talker's two settings, and the rooms the
    session was recorded with."""

    def __init__(self, doc: dict, layout: str):
        sr.SPREAD_SLOTS.setdefault(3, (0, 64, 256))                     # clones.json has three accounts
        super().__init__(doc, layout)
        self.rooms = [list_room(**rm) for rm in self.rooms]
        by_name = lambda name: next(i for i, x in enumerate(self.rooms) if x["name"] == name.encode())
        for _label, name, links, off in doc["config"].get("extra_rooms", []):      # a room behind the shipped ones
            self.rooms.append(list_room(name.encode(), desc=b"A %s off the %s.\n" % (name.encode(), off.encode()),
                                        links=[by_name(l) for l in (off,)]))
            self.rooms[by_name(off)]["links"].append(len(self.rooms) - 1)
        for name, service in doc["config"].get("netlinks", []):         # links nobody dials: unconnected
            self.rooms[by_name(name)]["netlink"] = (service.encode(), False, device.LINK_DOWN)
        self.gatecrash = int(doc["config"].get("gatecrash_level", ARCH))
        self.min_private = int(doc["config"].get("min_private", 2))

    def login(self, actor: str, name: str) -> None:
        super().login(actor, name)
        self.users[self.seats[actor]]["invite"] = None

    def everyone(self) -> dict:
        out = super().everyone()
        for u in out.values():
            u.setdefault("invite", None)
            u.setdefault("in_phrase", b"enters")
            u.setdefault("out_phrase", b"goes")
        return out

    def has_room_access(self, u: dict, rm: int) -> bool:
        return has_room_access(u, self.rooms, rm, self.gatecrash)


class GoModelBackend(sr.ModelBackend):
    def look(self, slot: int) -> bytes:
        return b"".join(look_of(self.all, self.st.rooms, slot))

    def go(self, slot: int, inpstr: bytes, word_count: int) -> dict:
        """One event through the model.  It changes ``self.all`` and the state's rooms as the move does, and returns
        the event's result with its plans as chunks."""
        st = self.st
        call = go_call(self.all, st.rooms, st.records(), [(slot, inpstr, word_count)], st.gatecrash, st.min_private)
        res = call["events"][0]
        for rm in call["cleared"]:
            self.rings.clear(rm)
        look = b"".join(res["look"]) if res["outcome"] in MOVED else None
        return {"outcome": res["outcome"], "target": res["target"], "old": res["old"], "returned": res["returned"], "look": look,
                "texts": {kind: res[kind] for kind in ("enter", "leave", "reset", "reply")},
                "plans": {kind: {"admitted": res["plans"][kind], "chunks": sr.both(res[kind])} for kind in res["plans"]}}


class GoDeviceBackend(sr.UploadingBackend):
    """One roster for the session; ``sync`` also uploads the phrases, the invites and the rooms' access."""

    def __init__(self, st):
        super().__init__(st)
        set_rooms(self.roster, st.rooms)
        self.sent_access = [rm["access"] for rm in st.rooms]

    def sync(self) -> None:
        now = self.st.everyone()
        for slot, u in now.items():
            was = self.sent.get(slot, {})
            changed = {f: u[f] for f in ("in_phrase", "out_phrase", "invite", "afk") if was.get(f, "unset") != u[f]}
            if changed:
                if "invite" in changed:
                    changed["invite_room"] = changed.pop("invite")
                self.roster.update(slot, **changed)
        super().sync()
        for slot, u in now.items():
            self.sent[slot].update({f: u[f] for f in ("in_phrase", "out_phrase", "invite", "afk")})
        for r, rm in enumerate(self.st.rooms):
            if rm["access"] != self.sent_access[r]:
                self.roster.set_rooms(r, access=rm["access"])
                self.sent_access[r] = rm["access"]

    def go(self, slot: int, inpstr: bytes, word_count: int) -> dict:
        st = self.st
        got = self.roster.go_many([(slot, inpstr, word_count)], gatecrash_level=st.gatecrash, min_private_users=st.min_private)
        self._count("go_many")
        outcome = int(got.outcome[0])
        if outcome in MOVED:                                            # the roster has applied the move: so does the state
            res = {"slot": slot, "target": int(got.target[0]), "old": int(got.old_room[0]), "returned": bool(got.returned_public[0]),
                   "look": None}
            apply_move(st.users, st.rooms, res, [])
            self.sent[slot]["room"] = st.users[slot]["room"]
            for j, u in st.users.items():
                self.sent[j]["invite"] = u["invite"]
            self.sent_access = [rm["access"] for rm in st.rooms]
        plans = {kind: plan_of(plan, 0) for kind, plan, _ in texts_of(got)}
        texts = {kind: text(0) or None for kind, _, text in texts_of(got)}
        return {"outcome": outcome, "target": int(got.target[0]), "old": int(got.old_room[0]), "returned": bool(got.returned_public[0]),
                "look": got.look.output(0) if got.look is not None else None, "texts": texts, "plans": plans}


class GoReplayer(sr.Replayer):
    """The Replayer with ``.go`` answered: the outcome, the texts and the look come from the backend's ``go``, nothing of
    them from the recording, and the mover's own bytes are compared.  ``.private``, ``.public`` and ``.invite`` are
    composed here from the reference's format strings, where the actor's bytes say that they took effect; the commands
    of STATE_ONLY -- the sessions of the other calls' tests hold some -- change the state where a later ``.go`` could
    see it and are compared with nothing.  Every other line is ``sr.Replayer``'s: it answers ``.clone``, ``.ignall``
    and the rest through the Roster's own event calls, and ``UploadingBackend`` then uploads the same state again."""
    STATE_ONLY = ("topic", "write", "rmst", "rmsn", "afk", "myclones", "switch", "inphr", "outphr", "desc")

    def __init__(self, doc: dict, backend_class=GoModelBackend, layout: str = sr.COMPACT):
        self._begin(doc, GoState(doc, layout), backend_class)
        self.res.update(go=0, go_outcomes={}, state_only=0, go_not_dispatched=0)

    def _go(self, u: dict, inp: dict, out: dict) -> None:
        st, slot, com = self.st, u["slot"], inp["com"]
        colour_before = {j: x["colour"] for j, x in st.users.items()}
        self.backend.sync()
        g = self.backend.go(slot, inp["inpstr"], inp["word_count"])
        self.res["go"] += 1
        self.res["go_outcomes"][g["outcome"]] = self.res["go_outcomes"].get(g["outcome"], 0) + 1
        if g["outcome"] == device.GO_NETLINK:
            return
        moved = g["outcome"] in MOVED
        if moved:
            u["went"] = True
        # the three room texts reach the clones' owners through relay_many, against the roster before the move: the relay
        # of the enter and the leave line is asked for before the backend moved, so it is composed here, from the records
        def room_text(kind, rm, sender):
            if g["texts"][kind] is None:
                return
            for j in g["plans"][kind]["admitted"]:
                if j in st.users:
                    out[j] += b"".join(g["plans"][kind]["chunks"][colour_before[j]])
            ignall = {j: x["ignall"] for j, x in st.everyone().items()}
            for c in sr.relays(st.records(), ignall, rm, None, g["texts"][kind]):
                owner = st.clones[c][0]
                out[owner] += b"".join(nuts_path.chunks(sr.relay_text(st.rooms[rm]["name"], g["texts"][kind]), st.users[owner]["colour"]))

        room_text("enter", g["target"], None)
        room_text("leave", g["old"], slot)
        if moved:
            out[slot] += g["look"]
        room_text("reset", g["old"], slot)
        if g["texts"]["reply"] is not None:
            out[slot] += b"".join(g["plans"]["reply"]["chunks"][u["colour"]])

    def _access(self, what: str, u: dict, inp: dict, out: dict, mine: str) -> bool:
        """.private, .public and .invite where they succeed, from the reference's format strings (c:4590-4611, 4687-4692);
        False where the actor's bytes say they did not."""
        st, slot, rm, com = self.st, u["slot"], u["room"], inp["com"]
        shown = u["name"] if u["vis"] else device.INVISNAME
        send = lambda j, text: out.__setitem__(j, out[j] + nuts_path.transduce(text, st.users[j]["colour"]))
        if what == "invite":
            if INVITE_LINE not in mine:
                return False
            who = sr.get_user(st.users, sr.capitalised(sr.words_of(inp["inpstr"])[0]))
            send(slot, b"You invite %s in.\n" % st.users[who]["name"])
            send(who, b"%s has invited you into the %s.\n" % (shown, st.rooms[rm]["name"]))
            st.users[who]["invite"] = rm
            return True
        word = b"~FRPRIVATE" if what == "private" else b"~FGPUBLIC"
        if "Room set to" not in mine or inp["word_count"] >= 2:
            return False
        send(slot, b"Room set to %s.\n" % word)
        self._broadcast(out, [(b"%s has set the room to %s.\n" % (shown, word), rm, slot, 0, com)])
        st.rooms[rm]["access"] = device.PRIVATE if what == "private" else device.PUBLIC
        if what == "public":
            for x in st.users.values():
                if x["invite"] == rm:
                    x["invite"] = None
            self.backend.rings.clear(rm) if hasattr(self.backend, "rings") else self.backend.roster.clear_review(rm)
        return True

    def _state_only(self, what: str, u: dict, inp: dict, mine: str) -> None:
        st, words = self.st, sr.words_of(inp["inpstr"])
        if what == "topic" and words:
            st.rooms[u["room"]]["topic"] = inp["inpstr"]
        elif what == "write" and words:
            st.rooms[u["room"]]["mesg_cnt"] += 1
        elif what == "afk":
            u["afk"] = 1
        elif what == "switch" and "strange sensation" in mine:           # clone_switch, c:7263-7290: the two change rooms
            i = st.find_clone(u["slot"], st.get_room(words[0]))
            st.clones[i][1], u["room"] = u["room"], st.clones[i][1]
        elif what == "inphr" and words:
            u["in_phrase"] = inp["inpstr"]
        elif what == "outphr" and words:
            u["out_phrase"] = inp["inpstr"]
        elif what == "desc" and words:
            u["desc"] = inp["inpstr"]

    def line(self, index: int, step: dict) -> None:
        st = self.st
        u = st.users[st.seats[step["actor"]]]
        data = step["send"].encode("latin-1") + b"\n"
        mine = step["recv"].get(step["actor"], "")
        if u.get("afk"):                                                # any input ends AFK (c:176-187): the line is not run
            u["afk"] = 0
            self.res["state_only"] += 1
            return
        self.backend.sync()
        inp = self.backend.input(u["slot"], data, record=False)
        what = nuts_path.lib().np_command_name(inp["com"]).decode() if inp["kind"] == sr.COMMAND else None
        if (step["send"].split() or [""])[0] == ".go" and what != "go":
            self.res["go_not_dispatched"] += 1                          # a NEW user's: exec_com answers "Unknown command."
        out = {slot: b"" for slot in st.users}
        if what in ("go", "private", "public", "invite"):
            netlinks = self.res["go_outcomes"].get(device.GO_NETLINK, 0)
            if what == "go":
                self._go(u, inp, out)
                if self.res["go_outcomes"].get(device.GO_NETLINK, 0) > netlinks:
                    return                                              # the netlink branch is the caller's: the outcome alone
            elif not self._access(what, u, inp, out, mine):
                self.res["state_only"] += 1
                return
            if u["command_mode"]:
                out[u["slot"]] += nuts_path.transduce(b"~FTCOM> " if u["vis"] else b"~FTCOM+> ", u["colour"])
            self.res["commands"][what] = self.res["commands"].get(what, 0) + 1
            self.res["answered"] += 1
            for actor, slot in st.seats.items():
                got, want = out[slot], step["recv"].get(actor, "").encode("latin-1")
                self.res["comparisons"] += 1
                if got != want:
                    self.res["mismatches"].append({"step": index, "send": step["send"][:80], "by": step["actor"], "client": actor,
                                                   "got": got.decode("latin-1")[:400], "want": want.decode("latin-1")[:400]})
        elif what in self.STATE_ONLY:
            self._state_only(what, u, inp, mine)
            self.res["state_only"] += 1
        else:
            super().line(index, step)

    def run(self) -> dict:
        try:
            for i, step in enumerate(self.doc["steps"]):
                if step["op"] == "login":
                    self.st.login(step["actor"], step["name"])
                elif step["op"] == "line":
                    self.line(i, step)
                elif step["op"] == "close":                             # the user leaves, and its clones with it
                    slot = self.st.seats.pop(step["actor"])
                    self.st.clones = [c for c in self.st.clones if c[0] != slot]
                    del self.st.users[slot]
                elif step["op"] not in ("connect", "dialog"):
                    raise sr.ReplayError(f"step {i}: a {step['op']!r} step")
        finally:
            self.backend.close()
        res = self.res
        res["slots"] = sorted(self.st.users)
        res["calls"] = getattr(self.backend, "calls", {})
        res["go_outcomes"] = {str(k): v for k, v in sorted(res["go_outcomes"].items())}
        return res


def go_lines(doc: dict) -> int:
    return lines_of(doc, ("go",))


def replay_sessions(backend_class=GoModelBackend, layouts=(sr.COMPACT,)) -> dict:
    out = {}
    for name in SESSIONS:
        doc = load(name)
        for layout in layouts:
            if layout == sr.SPREAD and len(doc["accounts"][0]) not in sr.SPREAD_SLOTS:
                continue
            res = GoReplayer(doc, backend_class, layout).run()
            out[f"{name}:{layout}"] = {"go": res["go"], "go_lines": go_lines(doc), "go_not_dispatched": res["go_not_dispatched"], "outcomes": res["go_outcomes"],
                                      "comparisons": res["comparisons"], "mismatches": res["mismatches"][:2],
                                      "n_mismatches": len(res["mismatches"]), "capacity": res["capacity"],
                                      "plan_disagreements": res["plan_disagreements"], "calls": res["calls"].get("go_many", 0)}
    return out


def parts(seed: int) -> tuple:
    return (("golden", lambda: replay_sessions(GoDeviceBackend, (sr.COMPACT, sr.SPREAD))), ("fuzz", lambda: fuzz_part(seed)),
            ("get_room", get_room_part), ("population", population_part), ("determinism", lambda: determinism_part(seed + 1)),
            ("regrown", lambda: regrown_part(seed + 2)), ("limits", limits_part))


def profile(res: dict) -> dict:
    return {"seconds": res["seconds"], "fuzz": {k: res["fuzz"][k] for k in ("calls", "events", "outcomes")},
            "golden": {k: {"go": v["go"], "comparisons": v["comparisons"]} for k, v in res["golden"].items()},
            "limits_seconds": res["limits"]["seconds"]}


def main() -> int:
    return child_main("DEVICE_GO", parts, profile, seed=20261)


if __name__ == "__main__":
    sys.exit(main())
