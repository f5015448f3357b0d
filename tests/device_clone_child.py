"""The device work of tests/test_device_clone.py, in a short-lived child process of its own, and the CPU model the host
tier of that module shares with it.

As tests/device_access_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_CLONE {...}``).  ``clone`` is the Python model of ``create_clone()``, ``destroy_clone()``,
``clone_say()`` and ``clone_hear()`` (nuts333.c:7100-7210, 7293-7357), built from the reference's format strings and with
``create_clone``'s loop over the user list transcribed as it stands; ``clone_call`` is the model of one ``Roster.clone_many``
call: it runs the events ONE AFTER ANOTHER, each against the state the earlier ones left, and defers by the rule of the
call -- so a device that decides every event against the snapshot agrees with it only if the rule makes the two the same.
``CloneReplayer`` answers the ``.clone``, ``.destroy``, ``.csay`` and ``.chear`` steps of the recorded sessions through a
backend's ``clone`` method, passes their room lines through ``relay`` and compares every client's bytes, the actor's
included.

    python tests/device_clone_child.py [--seed S]
"""
from __future__ import annotations

import random
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import session_replay as sr  # noqa: E402
from device_access_child import AccessDeviceBackend, AccessModelBackend, AccessReplayer  # noqa: E402
from device_go_child import (ARCH, WIZ, admitted, fuzz_rooms, fuzz_users, get_room, go_user, has_room_access, mirror_differences,  # noqa: E402
                             movers_of, seat, seat_clones, set_rooms)
from device_rooms_child import list_room  # noqa: E402
from device_tell_child import get_user  # noqa: E402
from event_checks import child_main, event_differences, lines_of, load, plan_of  # noqa: E402
from event_checks import digest as digest_of  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402

G = device
SESSIONS = ("reference_only/clone.json", "clones.json", "reference_only/access.json") + tuple(
    f"reference_only/replay_{seed}.json" for seed in sr.FIRST_SEEDS)
COMS = {"clone": G.COM_CLONE, "destroy": G.COM_DESTROY, "csay": G.COM_CSAY, "chear": G.COM_CHEAR}
EFFECTIVE = (G.CLONE_HEAR_NOTHING, G.CLONE_HEAR_SWEARS, G.CLONE_HEAR_ALL, G.CLONE_CREATED, G.CLONE_DESTROYED, G.CLONE_SAID)
KINDS = ("here", "there", "reset", "said", "reply", "notice")           # the rows of Clone.text_sizes
NOSUCHROOM, NOTLOGGEDON = b"There is no such room.\n", b"There is no one of that name logged on.\n"      # nuts333.h:145, 147
RESET_LINE = b"Room access returned to ~FGPUBLIC.\n"                    # c:2097
NO_CLONE = b"You do not have a clone in that room.\n"                   # c:7316, 7342
HEAR = {b"all": (G.CLONE_HEAR_ALL, b"Clone will now hear everything.\n"), b"swears": (G.CLONE_HEAR_SWEARS, b"Clone will now only hear swearing.\n"),
        b"nothing": (G.CLONE_HEAR_NOTHING, b"Clone will now hear nothing.\n")}
CAPACITIES = (1, 64, 65, 257)
EVENTS = (1, 8, 64)
WALK_CLONES = (1, 63, 64, 65, 255, 256, 257)


# ------------------------------------------------------------------ the model
def create_loop(rooms_of_mine: list, rm: int, max_clones: int) -> str:
    """create_clone's loop (c:7122-7135) as it stands, over the rooms of the actor's clones in list order."""
    cnt = 0
    for room in rooms_of_mine:
        if room == rm:
            return "already"
        cnt += 1
        if cnt == max_clones:
            return "maximum"
    return "created"


def create_rule(rooms_of_mine: list, rm: int, max_clones: int) -> str:
    """The same without the walk, as nuts_roster_clone decides: a min and two counts over the records."""
    m = next((i for i, room in enumerate(rooms_of_mine) if room == rm), None)
    before, total = (m if m is not None else 0), len(rooms_of_mine)
    if m is not None and (max_clones < 1 or before < max_clones):
        return "already"
    if max_clones >= 1 and total >= max_clones:
        return "maximum"
    return "created"


def find_clone(clones, owner: int, rm: int):
    return next((i for i, c in enumerate(clones) if c is not None and c[0] == owner and c[1] == rm), None)


def remaining(users: dict, clones, rm: int, but: int) -> int:
    """Who reset_access counts in rm (c:2095) once record ``but`` is gone: the users with a name and no login flag, the actor
    among them if it stands there, and the other clones."""
    return (sum(1 for u in users.values() if u["room"] == rm and u["name"] and not u["login"])
            + sum(1 for i, c in enumerate(clones) if c is not None and i != but and c[1] == rm))


def clone(users: dict, rooms, clones, slot: int, com: int, inpstr: bytes, wc: int, max_clones: int, gatecrash: int,
          min_private: int) -> dict:
    """What one ``.clone`` / ``.destroy`` / ``.csay`` / ``.chear`` does, without doing it: the outcome, the room, the slot
    and the record it resolved to, and the six texts."""
    u = users[slot]
    here = u["room"]
    res = {"slot": slot, "com": com, "outcome": None, "room": here, "target_room": -1, "target_slot": -1, "record": None,
           "returned": False, **{kind: None for kind in KINDS}}
    words = sr.words_of(inpstr)
    word1, word2 = (words + [b"", b""])[:2]
    me = u["name"]
    shown = me if u["vis"] else G.INVISNAME

    def done(outcome, reply, **more):
        res.update(outcome=outcome, reply=reply, **more)
        return res

    if com in (G.COM_CLONE, G.COM_DESTROY):
        rm = here
        if wc >= 2:
            rm = get_room(rooms, word1)
            if rm is None:
                return done(G.CLONE_NO_ROOM if com == G.COM_CLONE else G.CLONE_DESTROY_NO_ROOM, NOSUCHROOM)
        res["target_room"] = rm
        name = rooms[rm]["name"]
    if com == G.COM_CLONE:                                              # create_clone, c:7116-7160
        if not has_room_access(u, rooms, rm, gatecrash):
            return done(G.CLONE_PRIVATE, b"That room is currently private, you cannot create a clone there.\n")
        mine = [c[1] for c in clones if c is not None and c[0] == slot]
        verdict = create_loop(mine, rm, max_clones)
        if verdict == "already":
            return done(G.CLONE_ALREADY, b"You already have a clone in the %s.\n" % name, record=find_clone(clones, slot, rm))
        if verdict == "maximum":
            return done(G.CLONE_MAX, b"You already have the maximum number of clones allowed.\n")
        reply = (b"~FB~OLYou whisper a haunting spell and a clone is created here.\n" if rm == here
                 else b"~FB~OLYou whisper a haunting spell and a clone is created in the %s.\n" % name)
        return done(G.CLONE_CREATED, reply, here=b"~FB~OL%s whispers a haunting spell...\n" % shown,
                    there=b"~FB~OLA clone of %s appears in a swirling magical mist!\n" % me)
    if com == G.COM_DESTROY:                                            # destroy_clone, c:7179-7209
        whose = slot
        if wc > 2:
            whose = get_user(users, word2)
            if whose is None:
                return done(G.CLONE_DESTROY_NOBODY, NOTLOGGEDON)
            res["target_slot"] = whose
            if users[whose]["level"] >= u["level"]:
                return done(G.CLONE_DESTROY_LEVEL, b"You cannot destroy the clone of a user of an equal or higher level.\n")
        i = find_clone(clones, whose, rm)
        if i is None:
            if whose == slot:
                return done(G.CLONE_DESTROY_NONE_OWN, b"You do not have a clone in the %s.\n" % name)
            return done(G.CLONE_DESTROY_NONE_THEIRS, b"%s does not have a clone the %s.\n" % (users[whose]["name"], name))
        returned = rooms[rm]["access"] == G.PRIVATE and remaining(users, clones, rm, i) < min_private
        return done(G.CLONE_DESTROYED, b"~FM~OLYou whisper a sharp spell and the clone is destroyed.\n", record=i, returned=returned,
                    reset=RESET_LINE if returned else None, here=b"~FM~OL%s whispers a sharp spell...\n" % shown,
                    there=b"~FM~OLThe clone of %s shimmers and vanishes.\n" % users[whose]["name"],
                    notice=(b"~OLSYSTEM: ~FR%s has destroyed your clone in the %s.\n" % (me, name)) if whose != slot else None)
    if com == G.COM_CSAY:                                               # clone_say, c:7300-7316
        if u["muzzled"]:
            return done(G.CLONE_CSAY_MUZZLED, b"You are muzzled, your clone cannot speak.\n")
        if wc < 3:
            return done(G.CLONE_CSAY_USAGE, b"Usage: csay <room clone is in> <message>\n")
        rm = get_room(rooms, word1)
        if rm is None:
            return done(G.CLONE_CSAY_NO_ROOM, NOSUCHROOM)
        res["target_room"] = rm
        i = find_clone(clones, slot, rm)
        if i is None:
            return done(G.CLONE_CSAY_NONE, NO_CLONE)
        rest = nuts_path.lib().np_remove_first(inpstr)                  # say(u, remove_first(inpstr)), c:4080-4089
        return done(G.CLONE_SAID, None, record=i, said=b"Clone of %s %ss: %s\n" % (me, nuts_path.lib().np_say_verb(rest), rest))
    if wc < 3 or word2 not in HEAR:                                     # clone_hear, c:7328-7356
        return done(G.CLONE_CHEAR_USAGE, b"Usage: chear <room clone is in> all/swears/nothing\n")
    rm = get_room(rooms, word1)
    if rm is None:
        return done(G.CLONE_CHEAR_NO_ROOM, NOSUCHROOM)
    res["target_room"] = rm
    i = find_clone(clones, slot, rm)
    if i is None:
        return done(G.CLONE_CHEAR_NONE, NO_CLONE)
    return done(HEAR[word2][0], HEAR[word2][1], record=i)


def tail_of(clones) -> int:
    """The first record behind the last occupied one."""
    return max((i + 1 for i, c in enumerate(clones) if c is not None), default=0)


def clone_call(users: dict, rooms, clones: list, events, max_clones: int, gatecrash: int, min_private: int, rings=None) -> dict:
    """One clone_many call: the events one after another on ``clones`` -- a list of ``(owner, room, hear)`` or None, one per
    record -- and ``rooms`` and ``users``, which it changes.  An event is deferred when an earlier event of the call that
    was not deferred touched its owner slot -- the user get_user found, else the actor -- or the room its word resolved
    to; created and destroyed touch the owner and the room.  A destroyed record leaves the list as a node leaves the user
    list: the later ones move down.  A created one takes the first record behind the last occupied one of the call's
    start, moved down with the others.  Returns the events' results -- ``record`` an index into the records as they were
    before the call, ``created`` one into the records as they are after it -- with the plans of their texts, and the rooms
    whose review ring was cleared; ``rings`` records the said lines."""
    touched_rooms, touched_slots, out, cleared = set(), set(), [], []
    ids = list(range(len(clones)))                                      # where each record was before the call
    tail = tail_of(clones)
    for k, (slot, com, inpstr, wc) in enumerate(events):
        res = clone(users, rooms, clones, slot, com, inpstr, wc, max_clones, gatecrash, min_private)
        owner = res["target_slot"] if res["target_slot"] >= 0 else slot
        now = res["record"]
        res["record"] = -1 if now is None else ids[now]
        if owner in touched_slots or res["target_room"] in touched_rooms:
            res.update(outcome=G.CLONE_DEFERRED, returned=False, **{kind: None for kind in KINDS})
        rm = res["target_room"]
        res["plans"] = {"here": admitted(users, res["room"], slot) if res["here"] is not None else [],
                        "there": admitted(users, rm, slot if res["outcome"] == G.CLONE_CREATED else None) if res["there"] is not None else [],
                        "reset": admitted(users, rm, None) if res["reset"] is not None else [],
                        "said": admitted(users, rm, None) if res["said"] is not None else [],
                        "reply": [slot] if res["reply"] is not None else [],
                        "notice": [res["target_slot"]] if res["notice"] is not None else []}
        if res["outcome"] in (G.CLONE_HEAR_NOTHING, G.CLONE_HEAR_SWEARS, G.CLONE_HEAR_ALL):
            clones[now] = (clones[now][0], clones[now][1], res["outcome"])
        elif res["outcome"] == G.CLONE_SAID and rings is not None:
            rings.record(rm, res["said"])
        elif res["outcome"] == G.CLONE_CREATED:
            touched_slots.add(owner)
            touched_rooms.add(rm)
            clones[tail], ids[tail] = (slot, rm, G.CLONE_HEAR_ALL), ("new", k)
            tail += 1
        elif res["outcome"] == G.CLONE_DESTROYED:
            touched_slots.add(owner)
            touched_rooms.add(rm)
            del clones[now], ids[now]
            clones.append(None)
            ids.append(None)
            tail -= 1
            if res["returned"]:                                         # reset_access, c:2097-2104
                rooms[rm]["access"] = G.PUBLIC
                for x in users.values():
                    if x.get("invite") == rm:
                        x["invite"] = None
                cleared.append(rm)
                if rings is not None:
                    rings.clear(rm)
        out.append(res)
    for k, res in enumerate(out):
        res["created"] = ids.index(("new", k)) if res["outcome"] == G.CLONE_CREATED else -1
    return {"events": out, "cleared": cleared}


def texts_of(got: G.Clone):
    return (("here", got.here, got.here_text), ("there", got.there, got.there_text), ("reset", got.reset_plan, got.reset_text),
            ("said", got.said, got.said_text), ("reply", got.reply, got.reply_text), ("notice", got.notice, got.notice_text))


def clone_differences(got: G.Clone, call: dict) -> list:
    """Everything a Clone says against the model's call."""
    return event_differences(
        got, call, texts_of(got), G.CLONE_DEFERRED,
        lambda k, res: ((int(got.target_room[k]), int(got.target_slot[k]), int(got.record[k]), bool(got.reset[k]), int(got.created[k])),
                        (res["target_room"], res["target_slot"], res["record"], res["returned"], res["created"])),
        also_deferred=lambda k: got.reset[k] or got.created[k] != -1, effective=EFFECTIVE)


def record_differences(roster: G.Roster, clones) -> list:
    """The roster's clone mirrors against the model's records."""
    have = [None if o < 0 else (int(o), int(r), int(h)) for o, r, h in zip(roster._clone_owner, roster._clone_room, roster._clone_hear)]
    want = [None if c is None else tuple(c) for c in clones] + [None] * (roster.clones - len(clones))
    return [] if have == want else [{"what": "clone mirrors", "device": have[:12], "want": want[:12]}]


# ------------------------------------------------------------------ seeded streams
def clone_events(rng: random.Random, users: dict, rooms, clones, k: int) -> list:
    """Mixed events by users who may act; the words lean towards the rooms the actor has clones in.  word_count is the
    talker's: the command and the words of inpstr."""
    able = movers_of(users, len(rooms))
    named = [rm["name"] for rm in rooms if rm["name"]] or [b"none"]
    people = [u["name"] for u in users.values() if u["name"]]
    owners = sorted({c[0] for c in clones if c is not None} & set(able))
    events = []
    for _ in range(k):
        slot = rng.choice(owners) if owners and rng.random() < 0.6 else rng.choice(able)
        mine = [rooms[c[1]]["name"] for c in clones if c is not None and c[0] == slot and rooms[c[1]]["name"]]
        com = rng.choice((G.COM_CLONE, G.COM_CLONE, G.COM_DESTROY, G.COM_DESTROY, G.COM_CSAY, G.COM_CHEAR))
        kind = rng.random()
        room = (b"" if kind < 0.15 else rng.choice(mine) if kind < 0.55 and mine else rng.choice(named) if kind < 0.85
                else rng.choice(named)[:rng.randrange(1, 3)] if kind < 0.92 else rng.choice(named) + b"x")
        rest = b""
        if room and com == G.COM_DESTROY and rng.random() < 0.5:
            theirs = [users[c[0]]["name"] for c in clones if c is not None and users[c[0]]["name"]]
            pick = rng.random()
            rest = (rng.choice(theirs) if pick < 0.5 and theirs else rng.choice(people).lower() if pick < 0.7 else rng.choice(people)[:-1] or b"U"
                    if pick < 0.8 else users[slot]["name"] if pick < 0.9 else b"Nobody")
        elif room and com == G.COM_CSAY:
            rest = rng.choice((b"", b"hello", b"is it ~FGgreen?", b"look  out!", b"oh shit", b"\xe9t\xe9 ~OL!", b"x" * 900, b"a b c d e f g h i j k"))
        elif room and com == G.COM_CHEAR:
            rest = rng.choice((b"all", b"swears", b"nothing", b"All", b"al", b"", b"nothing more"))
        inpstr = room + (rng.choice((b" ", b"  ")) + rest if rest else b"") + rng.choice((b"", b"", b" "))
        events.append((slot, com, inpstr, min(G.MAX_WORDS, 1 + len(sr.words_of(inpstr)))))
    return events


def fuzz_clones(rng: random.Random, users: dict, nr: int, n: int) -> list:
    able = movers_of(users, nr)
    crowd = max(1, min(nr, 6))
    out = [(rng.choice(able[:24]), rng.randrange(crowd), rng.randrange(3)) if rng.random() < 0.7 else None for _ in range(n // 2)]
    return out + [None] * (n - len(out))


def trim(events, clones) -> list:
    """The events without the .clone events the records behind the last occupied one have no room for."""
    room, out = len(clones) - tail_of(clones), []
    for ev in events:
        if ev[1] == G.COM_CLONE:
            if not room:
                continue
            room -= 1
        out.append(ev)
    return out or [events[0][:1] + (G.COM_CHEAR,) + events[0][2:]]


def settings(rng: random.Random) -> tuple:
    return (rng.choice((0, 1, 2, 3, 2**31 - 1)), rng.randrange(G.MAX_LEVEL + 1), rng.choice((0, 1, 2, 3, 5, 2**31 - 1)))


def fuzz_part(seed: int, on_device: bool = True) -> dict:
    """Seeded streams of K = 1, 8, 64 mixed events at every capacity; without ``on_device`` the model alone, for its outcomes."""
    rng = random.Random(seed)
    bad, outcomes, calls, events_n, returned = [], {}, 0, 0, 0
    for cap in CAPACITIES:
        nr = 6
        rooms, users = fuzz_rooms(rng, nr), fuzz_users(rng, cap, nr)
        for u in users.values():
            u["muzzled"] = int(rng.random() < 0.1)
        if not movers_of(users, nr):
            users[0].update(name=b"U0", login=0, room=0)
        clones = fuzz_clones(rng, users, nr, 24)
        rings = sr.Rings(nr)
        if on_device:
            roster = G.Roster(cap, look_rooms=nr, clones=len(clones), review_rooms=nr)
            set_rooms(roster, rooms)
            seat(roster, users)
            roster.update(sorted(users), muzzled=[users[j]["muzzled"] for j in sorted(users)])
            seat_clones(roster, clones)
        for k in EVENTS:
            for _ in range(2):
                events = trim(clone_events(rng, users, rooms, clones, k), clones)
                max_clones, gatecrash, min_private = settings(rng)
                call = clone_call(users, rooms, clones, events, max_clones, gatecrash, min_private, rings)
                if on_device:
                    got = roster.clone_many(events, max_clones=max_clones, gatecrash_level=gatecrash, min_private_users=min_private,
                                            record=True)
                    found = clone_differences(got, call) + mirror_differences(roster, users, rooms) + record_differences(roster, clones)
                    rv = roster.review_many(list(range(nr)))
                    found += [{"what": "ring", "room": r} for r in range(nr) if rv.chunks(r, 1) != rings.chunks(r, 1)]
                    bad += [{"cap": cap, "k": k, **b} for b in found]
                calls += 1
                events_n += len(events)
                returned += sum(r["returned"] for r in call["events"])
                for r in call["events"]:
                    outcomes[r["outcome"]] = outcomes.get(r["outcome"], 0) + 1
        if on_device:
            roster.close()
    return {"capacities": list(CAPACITIES), "events_per_call": list(EVENTS), "calls": calls, "events": events_n, "returned_public": returned,
            "outcomes": {str(k): v for k, v in sorted(outcomes.items())}, "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ the record walk and the head-count, at the edges
def walk_positions(n: int) -> list:
    """The first and the last record, and both sides of 63/64 and 255/256: the edges of a lane, a wave and a block."""
    return sorted({p for p in (0, 62, 63, 64, 65, 254, 255, 256, n - 1) if 0 <= p < n})


def walk_tables() -> list:
    """``(records, filled)`` of every table of walk_part: for each n of WALK_CLONES a full table of n records, on which
    nothing can be created, and for the ``.clone`` cases, which the binding takes only with an empty record behind the last
    occupied one, a table of n records with the last one empty and one of n + 1 records with n filled."""
    return [t for n in WALK_CLONES for t in ((n, n), (n, n - 1), (n + 1, n))]


def walk_part() -> dict:
    """Hand-built tables (walk_tables).  The owner's records sit at walk_positions of the filled ones, all in the hall but
    one in the den; every other filled record is another owner's, in the den.  On a table with an empty record, ``.clone
    den`` with max_clones making the matching record the last one allowed (already) and the first one not (maximum), and
    past the owner's count (created when nothing matches), for the match at every position.  On a full table, ``.destroy
    den`` in a PRIVATE den whose head-count is the two users and the other owner's records, at min_private_users one below,
    at and above it, and a ``.csay`` and a ``.chear`` through the record."""
    bad, tables = [], []
    rooms0 = [list_room(b"den", links=[1], access=G.PRIVATE), list_room(b"hall", links=[0])]
    users0 = {0: go_user(0, name=b"Owner", room=1, level=ARCH, muzzled=0), 63: go_user(63, name=b"Other", room=0, level=ARCH, muzzled=0),
              64: go_user(64, name=b"Guest", room=0, muzzled=0), 256: go_user(256, name=b"Prompt", room=0, login=1, muzzled=0)}
    for records, filled in walk_tables():
        roster = G.Roster(257, look_rooms=2, clones=records)
        set_rooms(roster, rooms0)
        seat(roster, users0)
        spots, cases = walk_positions(filled), 0
        for at in spots or [None]:
            base = [(0, 1, G.CLONE_HEAR_ALL) if p in spots else (63, 0, G.CLONE_HEAR_ALL) for p in range(filled)] + [None] * (records - filled)
            if at is not None:
                base[at] = (0, 0, G.CLONE_HEAR_ALL)
            before = spots.index(at) if spots else 0
            others = sum(1 for c in base if c is not None and c[0] == 63)
            if records > filled:
                todo = [(G.COM_CLONE, b"den", m, 2) for m in (0, before, before + 1, len(spots), len(spots) + 1)]
            else:
                todo = ([(G.COM_DESTROY, b"den", 2, others + 2 + d) for d in (-1, 0, 1)]
                        + [(G.COM_CSAY, b"den hi", 2, 2), (G.COM_CHEAR, b"den swears", 2, 2)])
            for com, inpstr, max_clones, min_private in todo:
                users, rooms, clones = {j: dict(u) for j, u in users0.items()}, [dict(r) for r in rooms0], list(base)
                set_rooms(roster, rooms)
                seat_clones(roster, clones)
                events = [(0, com, inpstr, 1 + len(sr.words_of(inpstr)))]
                call = clone_call(users, rooms, clones, events, max_clones, ARCH, min_private)
                got = roster.clone_many(events, max_clones=max_clones, gatecrash_level=ARCH, min_private_users=min_private)
                found = clone_differences(got, call) + mirror_differences(roster, users, rooms) + record_differences(roster, clones)
                bad += [{"records": records, "filled": filled, "at": at, "com": com, "max_clones": max_clones, "min_private": min_private,
                         "seen_by_the_kernel": roster.clones, **b} for b in found]
                cases += 1
        tables.append([roster.clones, filled, cases])
        roster.close()
    return {"tables": tables, "cases": sum(t[2] for t in tables), "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ deferral, repeatability, regrowth
def same_owner_part() -> dict:
    """One call with the same owner and room in every event: all but the first defer."""
    rooms = [list_room(b"den", links=[1]), list_room(b"hall", links=[0])]
    users = {0: go_user(0, name=b"Owner", room=0, level=ARCH, muzzled=0), 1: go_user(1, name=b"Guest", room=1, muzzled=0)}
    clones = [None] * 8
    roster = G.Roster(2, look_rooms=2, clones=8)
    set_rooms(roster, rooms)
    seat(roster, users)
    events = [(0, G.COM_CLONE, b"hall", 2)] * 8
    call = clone_call(users, rooms, clones, events, 0, ARCH, 2)
    got = roster.clone_many(events, max_clones=0, gatecrash_level=ARCH, min_private_users=2)
    bad = clone_differences(got, call) + record_differences(roster, clones)
    roster.close()
    return {"outcomes": got.outcome.tolist(), "n_bad": len(bad), "first_bad": bad[:2]}


def digest(got: G.Clone) -> str:
    return digest_of(got, [got.target_room, got.target_slot, got.record, got.created, got.reset], texts_of(got))


def stream(seed: int, cap: int, k: int):
    rng = random.Random(seed)
    rooms, users = fuzz_rooms(rng, 6), fuzz_users(rng, cap, 6)
    for u in users.values():
        u["muzzled"] = 0
    if not movers_of(users, 6):
        users[0].update(name=b"U0", login=0, room=0)
    clones = fuzz_clones(rng, users, 6, 2 * k + 16)
    return rng, rooms, users, clones, trim(clone_events(rng, users, rooms, clones, k), clones)


def determinism_part(seed: int) -> dict:
    runs = []
    for _ in range(2):
        _, rooms, users, clones, events = stream(seed, 257, 64)
        roster = G.Roster(257, look_rooms=6, clones=len(clones))
        pair = []
        for _ in range(2):
            set_rooms(roster, rooms)                                    # back to the access, the invitations and the records before
            seat(roster, users)
            roster.set_clones(list(range(len(clones))), owner=None)
            seat_clones(roster, clones)
            pair.append(digest(roster.clone_many(events, max_clones=2, gatecrash_level=ARCH, min_private_users=2)))
        runs.append(pair)
        roster.close()
    return {"same_on_a_second_call": runs[0][0] == runs[0][1], "same_on_a_second_roster": runs[0] == runs[1]}


def regrown_part(seed: int) -> dict:
    """A small call that changes nothing, then one large enough to make the roster's device allocation grow: the table is
    not dirty, and has to travel again from the pinned mirror; then a relay_many and an access_many, which see the records."""
    cap = 65
    rng, rooms, users, clones, events = stream(seed, cap, 600)
    roster = G.Roster(cap, look_rooms=6, clones=len(clones))
    set_rooms(roster, rooms)
    seat(roster, users)
    seat_clones(roster, clones)
    actor = movers_of(users, 6)[0]
    kw = {"max_clones": 3, "gatecrash_level": ARCH, "min_private_users": 2}
    small = roster.clone_many([(actor, G.COM_CSAY, b"", 1)], **kw)
    clean = not (roster._dirty or roster._go_dirty or roster._rooms_dirty or roster._speech_dirty or roster._clones_dirty)
    call = clone_call(users, rooms, clones, events, 3, ARCH, 2)
    big = roster.clone_many(events, **kw)
    bad = clone_differences(big, call) + mirror_differences(roster, users, rooms) + record_differences(roster, clones)
    text = b"after the ~FRclones~RS\n"
    ignall = {j: u["ignall"] for j, u in users.items()}
    records = [(None, None, None) if c is None else c for c in clones]
    for rm in range(6):
        rl = roster.relay_many([(text, rm, None, 0, G.COM_SAY)])
        if rl.relays(0).tolist() != sr.relays(records, ignall, rm, None, text):
            bad.append({"what": "relay_many after", "room": rm, "device": rl.relays(0).tolist()[:10]})
    roster.close()
    return {"small_outcome": int(small.outcome[0]), "clean_before": clean, "small_h2d": small.timing["h2d_bytes"],
            "big_h2d": big.timing["h2d_bytes"], "capacity": cap, "events": len(events), "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ the recorded sessions
def pad(st) -> list:
    return st.records() + [None] * (st.clone_seats - len(st.clones))


def unpad(st, clones) -> None:
    st.clones = [list(c) for c in clones if c is not None]


class CloneModelBackend(AccessModelBackend):
    def clone(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        """One event through the model.  It changes the state's clones and rooms as the event does."""
        st = self.st
        clones = pad(st)
        call = clone_call(self.all, st.rooms, clones, [(slot, com, inpstr, word_count)], st.max_clones, st.gatecrash, st.min_private,
                          self.rings)
        unpad(st, clones)
        res = call["events"][0]
        for j, u in st.users.items():                                   # self.all holds copies of the clones' slots alone
            u["invite"] = self.all[j]["invite"]
        return {"outcome": res["outcome"], "room": res["room"], "target_room": res["target_room"], "target_slot": res["target_slot"],
                "texts": {kind: res[kind] for kind in KINDS},
                "plans": {kind: {"admitted": res["plans"][kind], "chunks": sr.both(res[kind])} for kind in KINDS}, "mirror": []}


class CloneDeviceBackend(AccessDeviceBackend):
    """One roster for the session.  After a ``clone_many`` the replayer's state takes the event's changes from what the
    call returned and is marked as sent: ``sync`` uploads nothing of them, and the roster's clone mirrors must equal it."""

    def clone(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        st = self.st
        got = self.roster.clone_many([(slot, com, inpstr, word_count)], max_clones=st.max_clones, gatecrash_level=st.gatecrash,
                                     min_private_users=st.min_private, record=True)
        self._count("clone_many")
        outcome, rm, rec = int(got.outcome[0]), int(got.target_room[0]), int(got.record[0])
        if outcome <= G.CLONE_HEAR_ALL:
            st.clones[rec][2] = outcome
        elif outcome == G.CLONE_CREATED:
            st.clones.append([slot, rm, G.CLONE_HEAR_ALL])
        elif outcome == G.CLONE_DESTROYED:
            del st.clones[rec]
            if got.reset[0]:
                st.rooms[rm]["access"] = G.PUBLIC
                for u in st.users.values():
                    if u["invite"] == rm:
                        u["invite"] = None
                for j, u in st.users.items():
                    self.sent[j]["invite"] = u["invite"]
                self.sent_access = [r["access"] for r in st.rooms]
        self.sent_clones = pad(st)
        return {"outcome": outcome, "room": st.users[slot]["room"], "target_room": rm, "target_slot": int(got.target_slot[0]),
                "texts": {kind: text(0) or None for kind, _, text in texts_of(got)},
                "plans": {kind: plan_of(plan, 0) for kind, plan, _ in texts_of(got)}, "mirror": record_differences(self.roster, pad(st))}


class CloneReplayer(AccessReplayer):
    """The AccessReplayer with ``.clone``, ``.destroy``, ``.csay`` and ``.chear`` answered: the outcome and the texts come
    from the backend's ``clone``, nothing of them from the recording, and the actor's own bytes are compared.  The room
    lines reach the clones' owners through the backend's ``relay``, over the records as the call left them: a new clone
    relays the two lines of its own creation and a destroyed one relays nothing, and ``relay``'s plan of each line must
    equal the call's.  ``.muzzle`` and ``.unmuzzle`` change the state a ``.csay`` reads.  A line that is none of these, nor the
    AccessReplayer's, is ``sr.Replayer``'s, which answers it through the Roster's own calls."""
    STATE_ONLY = AccessReplayer.STATE_ONLY + ("muzzle", "unmuzzle")

    def __init__(self, doc: dict, backend_class=CloneModelBackend, layout: str = sr.COMPACT):
        super().__init__(doc, backend_class, layout)
        self.res.update(clone=0, clone_outcomes={}, clone_lines=0)

    def _state_only(self, what: str, u: dict, inp: dict, mine: str) -> None:
        if what in ("muzzle", "unmuzzle"):                              # c:6461-6537: a user of a lower level
            words = sr.words_of(inp["inpstr"])
            who = get_user(self.st.users, words[0]) if words else None
            if who is not None and self.st.users[who]["level"] < u["level"]:
                self.st.users[who]["muzzled"] = int(what == "muzzle")
            return
        super()._state_only(what, u, inp, mine)

    def _answer_clone(self, index: int, step: dict, u: dict, inp: dict, what: str) -> None:
        st, slot, com = self.st, u["slot"], inp["com"]
        out = {j: b"" for j in st.users}
        a = self.backend.clone(slot, com, inp["inpstr"], inp["word_count"])
        self.res["clone"] += 1
        self.res["clone_outcomes"][a["outcome"]] = self.res["clone_outcomes"].get(a["outcome"], 0) + 1
        for m in a["mirror"]:
            self.res["mismatches"].append({"step": index, "send": step["send"][:80], **m})
        self.backend.sync()                                             # the clones' slots, for the looks that follow
        rm = a["target_room"]

        def room_line(kind, to, sender):
            text = a["texts"][kind]
            if text is None:
                return
            part = self.backend.relay([(text, to, sender, 0, com)])[0]
            self.res["plan_checks"] += 1
            if (part["plan"]["admitted"], part["plan"]["chunks"]) != (a["plans"][kind]["admitted"], a["plans"][kind]["chunks"]):
                self.res["plan_disagreements"] += 1
            self._deliver(out, [{"plan": a["plans"][kind], "relays": part["relays"]}])
            if kind == "said":
                self._note_record(to, text)

        room_line("reset", rm, None)                                    # reset_access runs before anything is written
        if a["texts"]["reply"] is not None:
            out[slot] += b"".join(a["plans"]["reply"]["chunks"][u["colour"]])
        room_line("here", a["room"], slot)
        room_line("there", rm, slot if a["outcome"] == G.CLONE_CREATED else None)
        if a["texts"]["notice"] is not None:
            who = a["target_slot"]
            out[who] += b"".join(a["plans"]["notice"]["chunks"][st.users[who]["colour"]])
        room_line("said", rm, None)
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
            self.res["clone_lines"] += 1
        if not u.get("afk"):
            self.backend.sync()
            inp = self.backend.input(u["slot"], step["send"].encode("latin-1") + b"\n", record=False)
            what = nuts_path.lib().np_command_name(inp["com"]).decode() if inp["kind"] == sr.COMMAND else None
            if what in COMS:
                self._answer_clone(index, step, u, inp, what)
                return
        super().line(index, step)


def clone_lines(doc: dict) -> int:
    return lines_of(doc, COMS)


def replay_sessions(backend_class=CloneModelBackend, layouts=(sr.COMPACT,)) -> dict:
    out = {}
    for name in SESSIONS:
        doc = load(name)
        for layout in layouts:
            if layout == sr.SPREAD and len(doc["accounts"][0]) not in sr.SPREAD_SLOTS:
                continue
            res = CloneReplayer(doc, backend_class, layout).run()
            out[f"{name}:{layout}"] = {"clone": res["clone"], "clone_lines": res["clone_lines"], "access": res["access"], "go": res["go"],
                                      "outcomes": {str(k): v for k, v in sorted(res["clone_outcomes"].items())},
                                      "comparisons": res["comparisons"], "mismatches": res["mismatches"][:2],
                                      "n_mismatches": len(res["mismatches"]), "capacity": res["capacity"], "plan_checks": res["plan_checks"],
                                      "plan_disagreements": res["plan_disagreements"], "calls": res["calls"].get("clone_many", 0)}
    return out


def parts(seed: int) -> tuple:
    return (("golden", lambda: replay_sessions(CloneDeviceBackend, (sr.COMPACT, sr.SPREAD))), ("fuzz", lambda: fuzz_part(seed)),
            ("walk", walk_part), ("same_owner", same_owner_part), ("determinism", lambda: determinism_part(seed + 1)),
            ("regrown", lambda: regrown_part(seed + 2)))


def profile(res: dict) -> dict:
    return {"seconds": res["seconds"], "fuzz": {k: res["fuzz"][k] for k in ("calls", "events", "outcomes")},
            "golden": {k: {"clone": v["clone"], "comparisons": v["comparisons"]} for k, v in res["golden"].items()},
            "walk_cases": res["walk"]["cases"], "walk_tables": res["walk"]["tables"]}


def main() -> int:
    return child_main("DEVICE_CLONE", parts, profile, seed=20263)


if __name__ == "__main__":
    sys.exit(main())
