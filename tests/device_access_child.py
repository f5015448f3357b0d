"""The device work of tests/test_device_access.py, in a short-lived child process of its own, and the CPU model the host
tier of that module shares with it.

As tests/device_go_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON line
it prints (``DEVICE_ACCESS {...}``).  ``access`` is the Python model of ``set_room_access()``, ``letmein()`` and
``invite()`` (nuts333.c:4543-4693), built from the reference's format strings; ``access_call`` is the model of one
``Roster.access_many`` call: it runs the events ONE AFTER ANOTHER, each against the state the earlier ones left, and defers
by the rule of the call -- so a device that decides every event against the snapshot agrees with it only if the rule makes
the two the same.  ``AccessReplayer`` answers the ``.public``, ``.private``, ``.letmein`` and ``.invite`` steps of the
recorded sessions through a backend's ``access`` method and compares every client's bytes, the actor's included.

    python tests/device_access_child.py [--seed S]
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
from device_go_child import (ARCH, EVENTS, WIZ, GoDeviceBackend, GoModelBackend, GoReplayer, admitted, cases,  # noqa: E402
                             first_word, fuzz_events, fuzz_rooms, fuzz_users, get_room, go_call, go_differences, go_user, look_of,
                             mirror_differences, movers_of, seat, seat_clones, set_rooms)
from device_rooms_child import list_room  # noqa: E402
from device_tell_child import get_user  # noqa: E402
from event_checks import child_main, event_differences, lines_of, load, plan_of  # noqa: E402
from event_checks import digest as digest_of  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402

G = device
SESSIONS = ("reference_only/access.json", "reference_only/go.json", "reference_only/rmst.json")
COMS = {"public": G.COM_PUBLIC, "private": G.COM_PRIVATE, "letmein": G.COM_LETMEIN, "invite": G.COM_INVITE}
EFFECTIVE = (G.ACCESS_SET_PRIVATE, G.ACCESS_SET_PUBLIC, G.ACCESS_INVITED)
KINDS = ("here", "there", "reply", "notice")
NOSUCHROOM, NOTLOGGEDON = b"There is no such room.\n", b"There is no one of that name logged on.\n"      # nuts333.h:145-146
EDGE_SLOTS = (0, 63, 64, 255, 256)


# ------------------------------------------------------------------ the model
def head_count(users: dict, clones, rm: int) -> int:
    """c:4583-4584: everybody in the user list whose room is rm -- the users with a name and no login flag, the actor among
    them, and the clones standing there."""
    return (sum(1 for u in users.values() if u["room"] == rm and u["name"] and not u["login"])
            + sum(1 for c in clones if c is not None and c[1] == rm))


def access(users: dict, rooms, clones, slot: int, com: int, inpstr: bytes, wc: int, gatecrash: int, min_private: int,
           ignore_mp: int) -> dict:
    """What one ``.public`` / ``.private`` / ``.letmein`` / ``.invite`` does, without doing it: the outcome, the room and the
    slot the word resolved to, and the four texts."""
    u = users[slot]
    here = u["room"]
    res = {"slot": slot, "com": com, "outcome": None, "room": here, "target_room": -1, "target_slot": -1, "here": None, "there": None,
           "reply": None, "notice": None}
    word = first_word(inpstr)
    shown = u["name"] if u["vis"] else G.INVISNAME

    def done(outcome, reply, **more):
        res.update(outcome=outcome, reply=reply, **more)
        return res

    if com in (G.COM_PUBLIC, G.COM_PRIVATE):                            # set_room_access, c:4551-4611
        rm = here
        if wc >= 2:
            if u["level"] < gatecrash:
                return done(G.ACCESS_LOW_LEVEL, b"You are not a high enough level to use the room option.\n")
            rm = get_room(rooms, word)
            if rm is None:
                return done(G.ACCESS_NO_ROOM, NOSUCHROOM)
        res["target_room"] = rm
        this = b"This" if rm == here else b"That"
        acc = rooms[rm]["access"]
        if acc > G.PRIVATE:
            return done(G.ACCESS_FIXED, this + b" room's access is fixed.\n")
        if com == G.COM_PUBLIC and acc == G.PUBLIC:
            return done(G.ACCESS_ALREADY_PUBLIC, this + b" room is already public.\n")
        if com == G.COM_PRIVATE:
            if acc == G.PRIVATE:
                return done(G.ACCESS_ALREADY_PRIVATE, this + b" room is already private.\n")
            if head_count(users, clones, rm) < min_private and u["level"] < ignore_mp:
                return done(G.ACCESS_TOO_FEW, b"You need at least %d users/clones in a room before it can be made private.\n" % min_private)
        to, outcome = (b"~FRPRIVATE", G.ACCESS_SET_PRIVATE) if com == G.COM_PRIVATE else (b"~FGPUBLIC", G.ACCESS_SET_PUBLIC)
        if rm == here:
            return done(outcome, b"Room set to %s.\n" % to, here=b"%s has set the room to %s.\n" % (shown, to))
        return done(outcome, b"Room set to %s.\n" % to, there=b"This room has been set to %s.\n" % to)
    if com == G.COM_LETMEIN:                                            # letmein, c:4622-4650
        if wc < 2:
            return done(G.ACCESS_LET_WHERE, b"Let you into where?\n")
        rm = get_room(rooms, word)
        if rm is None:
            return done(G.ACCESS_LET_NO_ROOM, NOSUCHROOM)
        res["target_room"] = rm
        name = rooms[rm]["name"]
        if rm == here:
            return done(G.ACCESS_LET_ALREADY, b"You are already in the %s!\n" % name)
        if rm not in rooms[here]["links"]:
            return done(G.ACCESS_LET_NOT_ADJOINED, b"The %s is not adjoined to here.\n" % name)
        if not rooms[rm]["access"] & G.PRIVATE:
            return done(G.ACCESS_LET_PUBLIC, b"The %s is currently public.\n" % name)
        return done(G.ACCESS_ASKED, b"You shout asking to be let into the %s.\n" % name,
                    here=b"%s shouts asking to be let into the %s.\n" % (u["name"], name),       # user->name, invisible or not
                    there=b"%s shouts asking to be let in.\n" % u["name"])
    if wc < 2:                                                          # invite, c:4662-4692
        return done(G.ACCESS_INVITE_WHO, b"Invite who?\n")
    if not rooms[here]["access"] & G.PRIVATE:
        return done(G.ACCESS_INVITE_PUBLIC, b"This room is currently public.\n")
    who = get_user(users, word)
    if who is None:
        return done(G.ACCESS_INVITE_NOBODY, NOTLOGGEDON)
    res["target_slot"] = who
    t = users[who]
    if who == slot:
        return done(G.ACCESS_INVITE_SELF, b"Inviting yourself to somewhere is the third sign of madness.\n")
    if t["room"] == here:
        return done(G.ACCESS_INVITE_HERE, b"%s is already here!\n" % t["name"])
    if t["invite"] == here:
        return done(G.ACCESS_INVITE_ALREADY, b"%s has already been invited into here.\n" % t["name"])
    return done(G.ACCESS_INVITED, b"You invite %s in.\n" % t["name"],
                notice=b"%s has invited you into the %s.\n" % (shown, rooms[here]["name"]))


def apply_access(users: dict, rooms, res: dict, cleared: list) -> None:
    """What an effective event changes (c:4596, 4605-4611, 4692)."""
    if res["outcome"] == G.ACCESS_INVITED:
        users[res["target_slot"]]["invite"] = res["room"]
    elif res["outcome"] == G.ACCESS_SET_PRIVATE:
        rooms[res["target_room"]]["access"] = G.PRIVATE
    elif res["outcome"] == G.ACCESS_SET_PUBLIC:
        rooms[res["target_room"]]["access"] = G.PUBLIC
        for x in users.values():
            if x.get("invite") == res["target_room"]:
                x["invite"] = None
        cleared.append(res["target_room"])


def access_call(users: dict, rooms, clones, events, gatecrash: int, min_private: int, ignore_mp: int) -> dict:
    """One access_many call: the events one after another on ``users`` and ``rooms``, which it changes.  An event is
    deferred when an earlier event of the call that was not deferred touched its actor's room, the room its word resolved
    to or the slot get_user found; set private and set public touch the room, invited touches the slot.  Returns the
    events' results with the plans of their texts, and the rooms whose review ring was cleared."""
    touched_rooms, touched_slots, out, cleared = set(), set(), [], []
    for slot, com, inpstr, wc in events:
        res = access(users, rooms, clones, slot, com, inpstr, wc, gatecrash, min_private, ignore_mp)
        if res["room"] in touched_rooms or res["target_room"] in touched_rooms or res["target_slot"] in touched_slots:
            res.update(outcome=G.ACCESS_DEFERRED, here=None, there=None, reply=None, notice=None)
        res["plans"] = {"here": admitted(users, res["room"], slot) if res["here"] is not None else [],
                        "there": admitted(users, res["target_room"], None) if res["there"] is not None else [],
                        "reply": [slot] if res["reply"] is not None else [],
                        "notice": [res["target_slot"]] if res["notice"] is not None else []}
        if res["outcome"] in (G.ACCESS_SET_PRIVATE, G.ACCESS_SET_PUBLIC):
            touched_rooms.add(res["target_room"])
        elif res["outcome"] == G.ACCESS_INVITED:
            touched_slots.add(res["target_slot"])
        apply_access(users, rooms, res, cleared)
        out.append(res)
    return {"events": out, "cleared": cleared}


def texts_of(got: G.Access):
    return (("here", got.here, got.here_text), ("there", got.there, got.there_text), ("reply", got.reply, got.reply_text),
            ("notice", got.notice, got.notice_text))


def access_differences(got: G.Access, call: dict) -> list:
    """Everything an Access says against the model's call."""
    return event_differences(
        got, call, texts_of(got), G.ACCESS_DEFERRED,
        lambda k, res: ((int(got.target_room[k]), int(got.target_slot[k])), (res["target_room"], res["target_slot"])), effective=EFFECTIVE)


# ------------------------------------------------------------------ seeded streams
def access_events(rng: random.Random, users: dict, rooms, k: int) -> list:
    able = movers_of(users, len(rooms))
    named = [rm["name"] for rm in rooms if rm["name"]] or [b"none"]
    people = [u["name"] for u in users.values() if u["name"]]
    events = []
    for _ in range(k):
        slot = rng.choice(able)
        here = rooms[users[slot]["room"]]
        com = rng.choice((G.COM_PUBLIC, G.COM_PRIVATE, G.COM_PRIVATE, G.COM_LETMEIN, G.COM_INVITE, G.COM_INVITE))
        kind = rng.random()
        if com == G.COM_INVITE:
            mates = [u["name"] for u in users.values() if u["name"] and u["room"] == users[slot]["room"]]
            invited = [u["name"] for u in users.values() if u["name"] and u["invite"] == users[slot]["room"] != u["room"]]
            word = (rng.choice(invited) if kind < 0.15 and invited else rng.choice(people) if kind < 0.5
                    else rng.choice(people).lower() if kind < 0.6 else rng.choice(people)[:-1] if kind < 0.7
                    else rng.choice(mates) if kind < 0.8 else users[slot]["name"] if kind < 0.85 else b"Nobody" if kind < 0.9
                    else b"n" * rng.choice((12, 13)) if kind < 0.95 else b"")
        else:
            linked = [rooms[l]["name"] for l in here["links"] if rooms[l]["name"]]
            word = (b"" if kind < 0.35 and com != G.COM_LETMEIN else rng.choice(linked) if kind < 0.6 and linked else rng.choice(named) if kind < 0.8
                    else rng.choice(named)[:rng.randrange(1, 3)] if kind < 0.88 else rng.choice(named) + b"x" if kind < 0.93
                    else here["name"] or b"x" if kind < 0.97 else b"")
        inpstr = rng.choice((b"", b" ", b"  ")) + word + rng.choice((b"", b"", b" now", b" \x01"))
        events.append((slot, com, inpstr, 1 if not word else rng.choice((2, 2, 2, 3))))
    return events


def settings(rng: random.Random) -> tuple:
    return (rng.randrange(G.MAX_LEVEL + 1), rng.choice((0, 1, 2, 2, 3, 5, 2**31 - 1)), rng.randrange(G.MAX_LEVEL + 2))


def following_differences(roster: G.Roster, users: dict, rooms, clones, ring_lines: dict, rng: random.Random) -> list:
    """A go_many, a look_many and a review_many after the call: they see the new state only if the binding applied it and
    the mirrors went up again."""
    bad = []
    event = fuzz_events(rng, users, rooms, 1)
    call = go_call(users, rooms, clones, event, ARCH, 2)
    got = roster.go_many(event, gatecrash_level=ARCH, min_private_users=2)
    bad += [{"after": "go_many", **b} for b in go_differences(got, call, users, rooms)]
    for rm in call["cleared"]:
        ring_lines[rm] = 0
    lookers = [j for j, u in users.items() if u["room"] is not None and u["room"] < len(rooms)][:8]
    if lookers:
        lk = roster.look_many(lookers)
        bad += [{"what": "look_many after", "slot": j} for i, j in enumerate(lookers) if lk.chunks(i) != look_of(users, rooms, j)]
    if roster.review_rooms:
        rings = list(range(roster.review_rooms))
        have = roster.review_many(rings).line_counts.tolist()
        if have != [ring_lines.get(r, 0) for r in rings]:
            bad.append({"what": "review_many after", "device": have, "want": [ring_lines.get(r, 0) for r in rings]})
    return bad


def fuzz_part(seed: int, on_device: bool = True) -> dict:
    """Seeded streams over every capacity and room count; without ``on_device`` the model alone, for its outcomes."""
    rng = random.Random(seed)
    bad, outcomes, calls, events_n = [], {}, 0, 0
    for cap, nr in cases():
        rooms, users = fuzz_rooms(rng, nr), fuzz_users(rng, cap, nr)
        if not movers_of(users, nr):
            users[0].update(name=b"U0", login=0, room=0)
        clones = [(rng.randrange(cap), rng.randrange(nr), 2) if rng.random() < 0.5 else None for _ in range(3)]
        ring_lines = {}
        if on_device:
            roster = G.Roster(cap, look_rooms=nr, clones=len(clones), review_rooms=min(nr, 4))
            set_rooms(roster, rooms)
            seat(roster, users)
            seat_clones(roster, clones)
        for k in EVENTS:
            events = access_events(rng, users, rooms, k)
            gatecrash, min_private, ignore_mp = settings(rng)
            if on_device:
                for rm in range(roster.review_rooms):                  # a line in every ring, for a set public to clear
                    roster.plan_many([(b"kept in the ring\n", rm, None, 0, G.COM_SAY)], record=True)
                    ring_lines[rm] = min(G.REVIEW_LINES, ring_lines.get(rm, 0) + 1)
            call = access_call(users, rooms, clones, events, gatecrash, min_private, ignore_mp)
            if on_device:
                got = roster.access_many(events, gatecrash_level=gatecrash, min_private_users=min_private, ignore_mp_level=ignore_mp)
                for rm in call["cleared"]:
                    ring_lines[rm] = 0
                found = access_differences(got, call) + mirror_differences(roster, users, rooms)
                found += following_differences(roster, users, rooms, clones, ring_lines, rng)
                bad += [{"cap": cap, "look_rooms": nr, "k": k, **b} for b in found]
            calls += 1
            events_n += k
            for r in call["events"]:
                outcomes[r["outcome"]] = outcomes.get(r["outcome"], 0) + 1
        if on_device:
            roster.close()
    return {"cases": [list(c) for c in cases()], "events_per_call": list(EVENTS), "calls": calls, "events": events_n,
            "outcomes": {str(k): v for k, v in sorted(outcomes.items())}, "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ head-count, get_user and get_room edges
def head_count_part() -> dict:
    """A public room with occupants at the edges of every lane, ballot word and block, the actor and one clone record: seven
    are counted; a login slot and a nameless slot of the room are not.  ``.private`` with min_private_users 7: in that room,
    and in one with one occupant fewer (no clone), by an actor below ignore_mp_level and by one at it."""
    out, bad = {}, []
    rooms0 = [list_room(b"den", links=[1]), list_room(b"hall", links=[0])]
    min_private = 7
    for label, actor_level, with_clone in (("exactly_enough", 1, True), ("one_fewer", 1, False), ("at_the_ignore_level", 2, False)):
        rooms = [dict(r) for r in rooms0]
        users = {j: go_user(j, name=b"U%d" % j, room=0, colour=j % 2) for j in EDGE_SLOTS}
        users[100] = go_user(100, name=b"Actor", room=0, level=actor_level)
        users[1] = go_user(1, name=b"Prompt", room=0, login=1)
        users[2] = go_user(2, name=None, room=0)
        users[3] = go_user(3, name=b"Guest", room=1)
        clones = [None, (3, 0, G.CLONE_HEAR_ALL) if with_clone else None, (3, 1, G.CLONE_HEAR_ALL)]
        roster = G.Roster(257, look_rooms=2, clones=3)
        set_rooms(roster, rooms)
        seat(roster, users)
        seat_clones(roster, clones)
        events = [(100, G.COM_PRIVATE, b"", 1)]
        counted = head_count(users, clones, 0)
        call = access_call(users, rooms, clones, events, ARCH, min_private, WIZ)
        got = roster.access_many(events, gatecrash_level=ARCH, min_private_users=min_private, ignore_mp_level=WIZ)
        bad += [{"part": label, **b} for b in access_differences(got, call) + mirror_differences(roster, users, rooms)]
        out[label] = {"outcome": int(got.outcome[0]), "counted": counted, "access": int(roster._room_rec[0, 21]),
                      "here_to": np.flatnonzero(got.here.admitted(0)).tolist(), "reply": got.reply_text(0).decode()}
        roster.close()
    return {**out, "n_bad": len(bad), "first_bad": bad[:2]}


GET_USER_WORDS = (b"anna", b"Anna", b"ann", b"abcdefghijkl", b"abcdefghijklm", b"bcdefghijkl", b"last", b"zan", b"Nna", b"host", b"prompt")


def get_user_part() -> dict:
    """Names at the edges; an exact match at slot 64 behind a substring match at slot 63; a login slot below both that
    holds the exact name; a 12-byte name; a 13-byte word."""
    rooms = [list_room(b"den", links=[1], access=G.PRIVATE), list_room(b"hall", links=[0])]
    users = {0: go_user(0, name=b"Zanna", room=1), 63: go_user(63, name=b"Annabel", room=1), 64: go_user(64, name=b"Anna", room=1),
             255: go_user(255, name=b"Abcdefghijkl", room=1), 256: go_user(256, name=b"Last", room=1),
             10: go_user(10, name=b"Anna", room=1, login=1), 11: go_user(11, name=None, room=1), 5: go_user(5, name=b"Host", room=0),
             6: go_user(6, name=b"Prompt", room=1, login=1)}
    roster = G.Roster(257, look_rooms=2)
    set_rooms(roster, rooms)
    seat(roster, users)
    targets, bad = [], []
    for w in GET_USER_WORDS:                                            # one event a call: every one is decided afresh
        events = [(5, G.COM_INVITE, w, 2)]
        call = access_call(users, rooms, [], events, ARCH, 2, WIZ)
        got = roster.access_many(events, gatecrash_level=ARCH, min_private_users=2, ignore_mp_level=WIZ)
        targets.append([int(got.outcome[0]), int(got.target_slot[0])])
        bad += [{"word": w.decode(), **b} for b in access_differences(got, call) + mirror_differences(roster, users, rooms)]
    invites = {j: int(roster._go_invite[j]) for j in sorted(users)}
    roster.close()
    return {"targets": targets, "invites": invites, "n_bad": len(bad), "first_bad": bad[:2]}


def get_room_part() -> dict:
    """The words of the go child's get_room_part, typed by an ARCH as ``.private <word>``."""
    out, bad = {}, []
    for label, nr, twins in (("255_256", 300, (255, 256)), ("0_1023", 1024, (0, 1023))):
        rooms = [list_room(b"n%d" % i, links=[]) for i in range(nr)]
        rooms[twins[0]]["name"], rooms[twins[1]]["name"] = b"twinroom_a", b"twinroom_b"
        rooms[3]["name"] = b"exactly_twenty_bytes"
        rooms[7]["name"] = b""                                          # a nameless room in between
        users = {0: go_user(0, name=b"Arch", room=5, level=ARCH)}
        roster = G.Roster(2, look_rooms=nr)
        set_rooms(roster, rooms)
        seat(roster, users)
        words = (b"twin", b"twinroom_b", b"twinroom_", b"exactly_twenty_bytes", b"exactly_twenty_bytesx", b"exactly_twenty_byte",
                 b"n7", b"n%d" % (nr - 1), b"twinroom_c")
        got_targets = []
        for w in words:
            events = [(0, G.COM_PRIVATE, w, 2)]
            call = access_call(users, rooms, [], events, ARCH, 2, WIZ)
            got = roster.access_many(events, gatecrash_level=ARCH, min_private_users=2, ignore_mp_level=WIZ)
            got_targets.append(int(got.target_room[0]))
            bad += [{"part": label, "word": w.decode(), **b} for b in access_differences(got, call) + mirror_differences(roster, users, rooms)]
        out[label] = got_targets
        roster.close()
    return {"targets": out, "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ repeatability, regrowth, limits
def digest(got: G.Access) -> str:
    return digest_of(got, [got.target_room, got.target_slot], texts_of(got))


def determinism_part(seed: int) -> dict:
    runs = []
    for _ in range(2):
        rng = random.Random(seed)
        rooms, users = fuzz_rooms(rng, 6), fuzz_users(rng, 257, 6)
        roster = G.Roster(257, look_rooms=6)
        set_rooms(roster, rooms)
        seat(roster, users)
        events = access_events(rng, users, rooms, 64)
        kw = {"gatecrash_level": ARCH, "min_private_users": 2, "ignore_mp_level": WIZ}
        first = digest(roster.access_many(events, **kw))
        seat(roster, users)                                             # back to the invitations and the access before
        set_rooms(roster, rooms)
        runs.append([first, digest(roster.access_many(events, **kw))])
        roster.close()
    return {"same_on_a_second_call": runs[0][0] == runs[0][1], "same_on_a_second_roster": runs[0] == runs[1]}


def regrown_part(seed: int) -> dict:
    """A small call that changes nothing, then one large enough to make the roster's device allocation grow: the table is
    not dirty, and has to travel again from the pinned mirror."""
    rng = random.Random(seed)
    cap, nr = 65, 6
    rooms, users = fuzz_rooms(rng, nr), fuzz_users(rng, cap, nr)
    roster = G.Roster(cap, look_rooms=nr)
    set_rooms(roster, rooms)
    seat(roster, users)
    actor = movers_of(users, nr)[0]
    kw = {"gatecrash_level": ARCH, "min_private_users": 2, "ignore_mp_level": WIZ}
    small = roster.access_many([(actor, G.COM_LETMEIN, b"", 1)], **kw)
    clean = not (roster._dirty or roster._go_dirty or roster._rooms_dirty or roster._speech_dirty)
    events = access_events(rng, users, rooms, 600)
    call = access_call(users, rooms, [], events, ARCH, 2, WIZ)
    big = roster.access_many(events, **kw)
    bad = access_differences(big, call) + mirror_differences(roster, users, rooms)
    bad += following_differences(roster, users, rooms, [], {}, rng)
    roster.close()
    return {"small_outcome": int(small.outcome[0]), "clean_before": clean, "small_h2d": small.timing["h2d_bytes"],
            "big_h2d": big.timing["h2d_bytes"], "capacity": cap, "events": len(events), "n_bad": len(bad), "first_bad": bad[:2]}


def limits_part() -> dict:
    """65,536 slots, 1,024 look rooms, 65,536 clone records, K = 64, against the model."""
    cap, nr, k = G.MAX_CAPACITY, G.MAX_LOOK_ROOMS, 64
    rng = np.random.default_rng(7)
    private = set(range(10, 16))
    rooms = [list_room(b"room%04d" % i, links=[(i + 1) % nr], access=G.PRIVATE if i in private else G.PUBLIC) for i in range(nr)]
    room = rng.integers(16, nr, cap).astype(np.int32)
    room[:32] = np.arange(32) // 2                                      # two users in each of the rooms 0 .. 15
    ids = list(range(cap))
    users = {j: go_user(j, name=b"U%d" % j, room=int(room[j]), level=1, colour=j & 1) for j in ids}
    roster = G.Roster(cap, look_rooms=nr, clones=G.MAX_CAPACITY)
    set_rooms(roster, rooms)
    roster.update(ids, room=room.tolist(), name=[b"U%d" % j for j in ids], level=1, colour=[j & 1 for j in ids])
    crooms = np.full(G.MAX_CAPACITY, 9, dtype=np.int32)
    crooms[-1] = 6                                                      # the last record stands in room 6
    roster.set_clones(list(range(G.MAX_CAPACITY)), owner=20, room=crooms.tolist())
    clones = [(20, int(r), G.CLONE_HEAR_ALL) for r in crooms]
    # .private by one of each pair (two users: too few, but in room 6, with the last clone, and in room 9); .letmein by the
    # other into the next room; invitations from the private rooms to the far end of the table; .public from the far end
    events = [(2 * i, G.COM_PRIVATE, b"", 1) for i in range(16)]
    events += [(2 * i + 1, G.COM_LETMEIN, b"room%04d" % (i + 1), 2) for i in range(16)]
    events += [(2 * i, G.COM_INVITE, b"u%d" % (cap - 1 - i), 2) for i in range(10, 16)] * 2
    events += [(cap - 1 - i, G.COM_PUBLIC, b"", 1) for i in range(k - len(events))]
    call = access_call(users, rooms, clones, events, ARCH, 3, WIZ)
    t0 = time.perf_counter()
    got = roster.access_many(events, gatecrash_level=ARCH, min_private_users=3, ignore_mp_level=WIZ)
    seconds = time.perf_counter() - t0
    bad = access_differences(got, call)
    want_invite = np.array([-1 if users[j]["invite"] is None else users[j]["invite"] for j in ids], dtype=np.int32)
    mirror_ok = bool((roster._go_invite == want_invite).all()) and [int(roster._room_rec[r, 21]) for r in range(nr)] == [rm["access"] for rm in rooms]
    privates = [r for r in range(16) if int(roster._room_rec[r, 21]) == G.PRIVATE]
    roster.close()
    return {"capacity": cap, "look_rooms": nr, "clones": G.MAX_CAPACITY, "k": len(events), "seconds": round(seconds, 3),
            "outcomes": sorted(set(got.outcome.tolist())), "mirror_ok": mirror_ok, "privates": privates,
            "invited": int((want_invite >= 0).sum()), "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ the recorded sessions
class AccessModelBackend(GoModelBackend):
    def access(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        """One event through the model.  It changes ``self.all`` and the state's rooms as the event does."""
        st = self.st
        call = access_call(self.all, st.rooms, st.records(), [(slot, com, inpstr, word_count)], st.gatecrash, st.min_private, st.ignore_mp)
        res = call["events"][0]
        for rm in call["cleared"]:
            self.rings.clear(rm)
        return {"outcome": res["outcome"], "room": res["room"], "target_room": res["target_room"], "target_slot": res["target_slot"],
                "texts": {kind: res[kind] for kind in KINDS},
                "plans": {kind: {"admitted": res["plans"][kind], "chunks": sr.both(res[kind])} for kind in KINDS}}


class AccessDeviceBackend(GoDeviceBackend):
    """One roster for the session.  After an ``access_many`` the replayer's state takes the event's changes and is marked
    as sent: nothing of them is uploaded by ``sync``, so a later ``.go`` or ``.review`` sees what the binding applied."""

    def access(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        st = self.st
        got = self.roster.access_many([(slot, com, inpstr, word_count)], gatecrash_level=st.gatecrash,
                                      min_private_users=st.min_private, ignore_mp_level=st.ignore_mp)
        self._count("access_many")
        res = {"outcome": int(got.outcome[0]), "room": st.users[slot]["room"], "target_room": int(got.target_room[0]),
               "target_slot": int(got.target_slot[0])}
        if res["outcome"] in EFFECTIVE:
            apply_access(st.users, st.rooms, res, [])
            for j, u in st.users.items():
                self.sent[j]["invite"] = u["invite"]
            self.sent_access = [rm["access"] for rm in st.rooms]
        return {**res, "texts": {kind: text(0) or None for kind, _, text in texts_of(got)},
                "plans": {kind: plan_of(plan, 0) for kind, plan, _ in texts_of(got)}}


class AccessReplayer(GoReplayer):
    """The GoReplayer with ``.public``, ``.private``, ``.letmein`` and ``.invite`` answered: the outcome and the texts come
    from the backend's ``access``, nothing of them from the recording, and the actor's own bytes are compared.  The two
    room lines reach the clones' owners as after ``go_many``: composed here from the clone records, as ``relay_many``
    relays them.  A line that is none of these four, nor the GoReplayer's, is ``sr.Replayer``'s, which answers it through the
    Roster's own calls."""

    def __init__(self, doc: dict, backend_class=AccessModelBackend, layout: str = sr.COMPACT):
        super().__init__(doc, backend_class, layout)
        self.st.ignore_mp = int(doc["config"].get("ignore_mp_level", WIZ))       # WIZ in every provisioned config
        self.res.update(access=0, access_outcomes={}, access_lines=0)

    def _answer(self, index: int, step: dict, u: dict, inp: dict, what: str) -> None:
        st, slot = self.st, u["slot"]
        out = {j: b"" for j in st.users}
        a = self.backend.access(slot, inp["com"], inp["inpstr"], inp["word_count"])
        self.res["access"] += 1
        self.res["access_outcomes"][a["outcome"]] = self.res["access_outcomes"].get(a["outcome"], 0) + 1
        if a["texts"]["reply"] is not None:                             # write_user(user, ...) comes first
            out[slot] += b"".join(a["plans"]["reply"]["chunks"][u["colour"]])
        ignall = {j: x["ignall"] for j, x in st.everyone().items()}
        for kind, rm in (("here", a["room"]), ("there", a["target_room"])):
            text = a["texts"][kind]
            if text is None:
                continue
            for j in a["plans"][kind]["admitted"]:
                if j in st.users:
                    out[j] += b"".join(a["plans"][kind]["chunks"][st.users[j]["colour"]])
            for c in sr.relays(st.records(), ignall, rm, None, text):
                owner = st.clones[c][0]
                out[owner] += b"".join(nuts_path.chunks(sr.relay_text(st.rooms[rm]["name"], text), st.users[owner]["colour"]))
        if a["texts"]["notice"] is not None:
            who = a["target_slot"]
            out[who] += b"".join(a["plans"]["notice"]["chunks"][st.users[who]["colour"]])
        if u["command_mode"]:
            out[slot] += nuts_path.transduce(b"~FTCOM> " if u["vis"] else b"~FTCOM+> ", u["colour"])
        self.res["commands"][what] = self.res["commands"].get(what, 0) + 1
        self.res["answered"] += 1
        for actor, j in st.seats.items():
            got, want = out[j], step["recv"].get(actor, "").encode("latin-1")
            self.res["comparisons"] += 1
            if got != want:
                self.res["mismatches"].append({"step": index, "send": step["send"][:80], "by": step["actor"], "client": actor,
                                               "got": got.decode("latin-1")[:400], "want": want.decode("latin-1")[:400]})

    def line(self, index: int, step: dict) -> None:
        st = self.st
        u = st.users[st.seats[step["actor"]]]
        if (step["send"].split() or [""])[0].lstrip(".") in COMS:
            self.res["access_lines"] += 1
        if not u.get("afk"):
            self.backend.sync()
            inp = self.backend.input(u["slot"], step["send"].encode("latin-1") + b"\n", record=False)
            what = nuts_path.lib().np_command_name(inp["com"]).decode() if inp["kind"] == sr.COMMAND else None
            if what in COMS:
                self._answer(index, step, u, inp, what)
                return
        super().line(index, step)


def access_lines(doc: dict) -> int:
    return lines_of(doc, COMS)


def replay_sessions(backend_class=AccessModelBackend, layouts=(sr.COMPACT,)) -> dict:
    out = {}
    for name in SESSIONS:
        doc = load(name)
        for layout in layouts:
            if layout == sr.SPREAD and len(doc["accounts"][0]) not in sr.SPREAD_SLOTS:
                continue
            res = AccessReplayer(doc, backend_class, layout).run()
            out[f"{name}:{layout}"] = {"access": res["access"], "access_lines": access_lines(doc), "go": res["go"],
                                      "outcomes": {str(k): v for k, v in sorted(res["access_outcomes"].items())},
                                      "comparisons": res["comparisons"], "mismatches": res["mismatches"][:2],
                                      "n_mismatches": len(res["mismatches"]), "capacity": res["capacity"],
                                      "plan_disagreements": res["plan_disagreements"], "calls": res["calls"].get("access_many", 0)}
    return out


def parts(seed: int) -> tuple:
    return (("golden", lambda: replay_sessions(AccessDeviceBackend, (sr.COMPACT, sr.SPREAD))), ("fuzz", lambda: fuzz_part(seed)),
            ("head_count", head_count_part), ("get_user", get_user_part), ("get_room", get_room_part),
            ("determinism", lambda: determinism_part(seed + 1)), ("regrown", lambda: regrown_part(seed + 2)), ("limits", limits_part))


def profile(res: dict) -> dict:
    return {"seconds": res["seconds"], "fuzz": {k: res["fuzz"][k] for k in ("calls", "events", "outcomes")},
            "golden": {k: {"access": v["access"], "comparisons": v["comparisons"]} for k, v in res["golden"].items()},
            "limits_seconds": res["limits"]["seconds"]}


def main() -> int:
    return child_main("DEVICE_ACCESS", parts, profile, seed=20262)


if __name__ == "__main__":
    sys.exit(main())
