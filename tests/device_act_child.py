"""The device work of tests/test_device_act.py, in a short-lived child process of its own, and the CPU model the host
tier of that module shares with it.

As tests/device_access_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_ACT {...}``).  ``act`` is the Python model of ``move()``, ``wake()``, ``muzzle()`` and
``unmuzzle()`` (nuts333.c:4726-4768, 6496-6522, 6571-6703) with teleport 2 of ``move_user`` (c:4409-4459), built from the
reference's format strings; ``act_call`` is the model of one ``Roster.act_many`` call: it runs the events ONE AFTER
ANOTHER, each against the state the earlier ones left, and defers by the rule of the call and by the binding's own -- so a
device that decides every event against the snapshot agrees with it only if the rule makes the two the same;
``apply_act`` applies an event's changes to the state.  ``ActReplayer`` answers the ``.move``, ``.wake``, ``.muzzle`` and
``.unmuzzle`` steps of the recorded sessions through a backend's ``act`` method and compares every client's bytes.

    python tests/device_act_child.py [--seed S]
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
from device_access_child import access_call, access_differences, access_events  # noqa: E402
from device_go_child import (ARCH, CAPACITIES, EVENTS, LOOK_ROOMS, WIZ, admitted, fuzz_events, fuzz_rooms, fuzz_users,  # noqa: E402
                             get_room, go_call, go_differences, go_user, has_room_access, look_of, mirror_differences,
                             movers_of, population, seat, seat_clones, set_rooms)
from device_rooms_child import list_room  # noqa: E402
from device_tell_child import get_user  # noqa: E402
from event_checks import child_main, event_differences, lines_of, load  # noqa: E402
from event_checks import digest as digest_of  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402

G = device
COMS = {"move": G.COM_MOVE, "wake": G.COM_WAKE, "muzzle": G.COM_MUZZLE, "unmuzzle": G.COM_UNMUZZLE}
MOVED = (G.ACT_MOVED, G.ACT_MOVED_UNSEEN)
EFFECTIVE = MOVED + (G.ACT_MUZZLED, G.ACT_UNMUZZLED)
KINDS = ("here", "enter", "leave", "reset", "reply", "notice")
NOSUCHROOM, NOTLOGGEDON = b"There is no such room.\n", b"There is no one of that name logged on.\n"      # nuts333.h:145-146
INVISENTER, INVISLEAVE = b"A presence enters the room...\n", b"A presence leaves the room.\n"
RESET_LINE = b"Room access returned to ~FGPUBLIC.\n"                                     # c:2097
USAGE = {G.COM_MOVE: (G.ACT_MOVE_USAGE, b"Usage: move <user> [<room>]\n"), G.COM_WAKE: (G.ACT_WAKE_USAGE, b"Usage: wake <user>\n"),
         G.COM_MUZZLE: (G.ACT_MUZZLE_USAGE, b"Usage: muzzle <user>\n"), G.COM_UNMUZZLE: (G.ACT_UNMUZZLE_USAGE, b"Usage: unmuzzle <user>\n")}
EDGE_SLOTS = (0, 63, 64, 255, 256)


# ------------------------------------------------------------------ the model
def act_user(slot: int, **fields) -> dict:
    """A go_user with ``muzzle``, the level byte 15 of its speaker row holds: 0 beside a set ``muzzled`` bit reads as WIZ."""
    return go_user(slot, **{"muzzle": 0, **fields})


def muzzle_of(u: dict) -> int:
    """user->muzzled as the kernel reads it of a slot."""
    return 0 if not u["muzzled"] else u.get("muzzle") or WIZ


def act(users: dict, rooms, clones, slot: int, com: int, inpstr: bytes, wc: int, gatecrash: int, min_private: int) -> dict:
    """What one ``.move`` / ``.wake`` / ``.muzzle`` / ``.unmuzzle`` does, without doing it: the outcome, the slot, the room
    and the room left that it resolved to, and the six texts."""
    u = users[slot]
    here = u["room"]
    res = {"slot": slot, "com": com, "outcome": None, "room": here, "target_slot": -1, "target_room": here, "old": -1, "returned": False,
           **{kind: None for kind in KINDS}}
    words = sr.words_of(inpstr)
    word1, word2 = (words + [b"", b""])[:2]
    shown = u["name"] if u["vis"] else G.INVISNAME

    def done(outcome, reply, **more):
        res.update(outcome=outcome, reply=reply, **more)
        return res

    if wc < 2:                                                          # c:4733, 6502, 6576, 6648
        return done(*USAGE[com])
    if com == G.COM_WAKE and u["muzzled"]:                              # c:6505
        return done(G.ACT_WAKE_MUZZLED, b"You are muzzled, you cannot wake anyone.\n")
    who = get_user(users, word1)
    t = users[who] if who is not None else None
    if who is not None:
        res.update(target_slot=who, old=-1 if t["room"] is None else t["room"])
    if com == G.COM_MOVE:                                               # c:4736-4766
        rm = here
        if wc >= 3:
            rm = get_room(rooms, word2) if who is not None else None
            res["target_room"] = -1 if rm is None else rm
        if who is None:
            return done(G.ACT_MOVE_NOBODY, NOTLOGGEDON)
        if rm is None:
            return done(G.ACT_MOVE_NO_ROOM, NOSUCHROOM)
        if who == slot:
            return done(G.ACT_MOVE_SELF, b"Trying to move yourself this way is the fourth sign of madness.\n")
        if t["level"] >= u["level"]:
            return done(G.ACT_MOVE_LEVEL, b"You cannot move a user of equal or higher level than yourself.\n")
        if rm == t["room"]:
            return done(G.ACT_MOVE_ALREADY, b"%s is already in the %s.\n" % (t["name"], rooms[rm]["name"]))
        if not has_room_access(u, rooms, rm, gatecrash):
            return done(G.ACT_MOVE_PRIVATE, b"The %s is currently private, %s cannot be moved there.\n" % (rooms[rm]["name"], t["name"]))
        if t["room"] is None or t["room"] >= len(rooms):
            return done(G.ACT_MOVE_AWAY, None)
        res["here"] = b"~FT~OL%s chants an ancient spell...\n" % shown
        if not t["vis"]:                                                # move_user, c:4423-4427
            res.update(enter=INVISENTER, leave=INVISLEAVE)
        else:                                                           # c:4435-4447
            res.update(notice=b"\n~FT~OLA giant hand grabs you and pulls you into a magical blue vortex!\n",
                       enter=b"~FT~OL%s falls out of a magical blue vortex!\n" % t["name"],
                       leave=b"~FT~OLA giant hand grabs %s who is pulled into a magical blue vortex!\n" % t["name"])
        if rooms[t["room"]]["access"] == G.PRIVATE and population(users, clones, t["room"], who) < min_private:
            res.update(returned=True, reset=RESET_LINE)
        return done(G.ACT_MOVED if t["vis"] else G.ACT_MOVED_UNSEEN, b"~FT~OLYou chant an ancient spell...\n")
    if com == G.COM_WAKE:                                               # c:6508-6521
        if who is None:
            return done(G.ACT_WAKE_NOBODY, NOTLOGGEDON)
        if who == slot:
            return done(G.ACT_WAKE_SELF, b"Trying to wake yourself up is the eighth sign of madness.\n")
        if t["afk"]:
            return done(G.ACT_WAKE_AFK, b"You cannot wake someone who is AFK.\n")
        return done(G.ACT_WOKEN, b"Wake up call sent.\n", notice=b"\07\n~BR*** %s says: ~OL~LIWAKE UP!!!~RS~BR ***\n\n" % shown)
    if com == G.COM_MUZZLE:                                             # c:6579-6598
        if who is None:
            return done(G.ACT_MUZZLE_ABSENT, None)
        if who == slot:
            return done(G.ACT_MUZZLE_SELF, b"Trying to muzzle yourself is the ninth sign of madness.\n")
        if t["level"] >= u["level"]:
            return done(G.ACT_MUZZLE_LEVEL, b"You cannot muzzle a user of equal or higher level than yourself.\n")
        if muzzle_of(t) >= u["level"]:
            return done(G.ACT_MUZZLE_ALREADY, b"%s is already muzzled.\n" % t["name"])
        return done(G.ACT_MUZZLED, b"~FR~OL%s now has a muzzle of level: ~RS~OL%s.\n" % (t["name"], G.LEVEL_NAMES[u["level"]]),
                    notice=b"~FR~OLYou have been muzzled!\n")
    if who is None:                                                     # c:6651-6669
        return done(G.ACT_UNMUZZLE_ABSENT, None)
    if who == slot:
        return done(G.ACT_UNMUZZLE_SELF, b"Trying to unmuzzle yourself is the tenth sign of madness.\n")
    if not muzzle_of(t):
        return done(G.ACT_UNMUZZLE_NOT, None)                           # c:6656-6658: sprintf, and no write
    if muzzle_of(t) > u["level"]:
        return done(G.ACT_UNMUZZLE_ABOVE, b"%s's muzzle is set to level %s, you do not have the power to remove it.\n"
                    % (t["name"], G.LEVEL_NAMES[muzzle_of(t)]))
    return done(G.ACT_UNMUZZLED, b"~FG~OLYou remove %s's muzzle.\n" % t["name"], notice=b"~FG~OLYou have been unmuzzled!\n")


def apply_act(users: dict, rooms, res: dict, cleared: list) -> None:
    """What an effective event changes: move_user's and reset_access's changes of state (c:4422, 4456, 2098-2104), with the
    target's look between the two kept in ``res``; the muzzle (c:6597, 6668)."""
    if res["outcome"] in MOVED:
        t = users[res["target_slot"]]
        if t["invite"] == res["target_room"]:
            t["invite"] = None
        t["room"] = res["target_room"]
        if "look" not in res:
            res["look"] = look_of(users, rooms, res["target_slot"])
        if res["returned"]:
            rooms[res["old"]]["access"] = G.PUBLIC
            for x in users.values():
                if x["invite"] == res["old"]:
                    x["invite"] = None
            cleared.append(res["old"])
    elif res["outcome"] == G.ACT_MUZZLED:
        users[res["target_slot"]].update(muzzled=1, muzzle=users[res["slot"]]["level"])
    elif res["outcome"] == G.ACT_UNMUZZLED:
        users[res["target_slot"]].update(muzzled=0, muzzle=0)


def act_call(users: dict, rooms, clones, events, gatecrash: int, min_private: int) -> dict:
    """One act_many call: the events one after another on ``users`` and ``rooms``, which it changes.  An event is deferred
    when an earlier event of the call that the rule did not defer touched its actor's slot, the slot get_user found, the
    actor's room, the found slot's room or the resolved room; a move touches the target's slot, the room left and the room
    entered, a muzzle set or removed the target's slot.  The binding's own: a move whose new room adjoins a room that an
    earlier event returned to public; the device has let such a move touch already, so it touches here as well.  Returns the events' results with the plans of their texts, the rooms whose review ring was
    cleared, and the moved targets in event order."""
    touched_slots, touched_rooms, out, cleared, movers = set(), set(), [], [], []
    for slot, com, inpstr, wc in events:
        res = act(users, rooms, clones, slot, com, inpstr, wc, gatecrash, min_private)
        who = res["target_slot"]
        by_rule = bool(slot in touched_slots or who in touched_slots or {res["room"], res["old"], res["target_room"]} & touched_rooms)
        if not by_rule and res["outcome"] in EFFECTIVE:
            touched_slots.add(who)
            if res["outcome"] in MOVED:
                touched_rooms |= {res["old"], res["target_room"]}
        if by_rule or (res["outcome"] in MOVED and set(cleared) & set(rooms[res["target_room"]]["links"])):
            res.update(outcome=G.ACT_DEFERRED, returned=False, **{kind: None for kind in KINDS})
        res["plans"] = {"here": admitted(users, res["room"], slot) if res["here"] is not None else [],
                        "enter": admitted(users, res["target_room"], None) if res["enter"] is not None else [],
                        "leave": admitted(users, res["old"], who) if res["leave"] is not None else [],
                        "reset": admitted(users, res["old"], who) if res["reset"] is not None else [],
                        "reply": [slot] if res["reply"] is not None else [],
                        "notice": [who] if res["notice"] is not None else []}
        if res["outcome"] in MOVED:
            movers.append(who)
        apply_act(users, rooms, res, cleared)
        out.append(res)
    return {"events": out, "cleared": cleared, "movers": movers}


def texts_of(got: G.Act):
    return (("here", got.here, got.here_text), ("enter", got.enter, got.enter_text), ("leave", got.leave, got.leave_text),
            ("reset", got.reset, got.reset_text), ("reply", got.reply, got.reply_text), ("notice", got.notice, got.notice_text))


def act_differences(got: G.Act, call: dict, users: dict) -> list:
    """Everything an Act says against the model's call; ``users`` is the state after it."""
    bad = event_differences(
        got, call, texts_of(got), G.ACT_DEFERRED,
        lambda k, res: ((int(got.target_slot[k]), int(got.target_room[k]), int(got.old_room[k]), bool(got.returned_public[k])),
                        (res["target_slot"], res["target_room"], res["old"], res["returned"])),
        also_deferred=lambda k: got.returned_public[k], effective=EFFECTIVE)
    movers = call["movers"]
    if (got.look is None) != (not movers) or got.moved().tolist() != [k for k, r in enumerate(call["events"]) if r["outcome"] in MOVED]:
        bad.append({"what": "movers", "device": got.moved().tolist()})
    elif movers:
        if got.look.slots.tolist() != movers or got.look_index[got.moved()].tolist() != list(range(len(movers))):
            bad.append({"what": "look slots", "device": got.look.slots.tolist(), "want": movers})
        else:
            looks = [r["look"] for r in call["events"] if r["outcome"] in MOVED]
            bad += [{"what": "look", "slot": slot, "room": users[slot]["room"]} for i, slot in enumerate(movers)
                    if got.look.chunks(i) != looks[i]]
    return bad


def muzzle_differences(roster: G.Roster, users: dict) -> list:
    """The muzzled bit and byte 15 of the speaker mirror against the model's state."""
    bad = []
    for j, u in users.items():
        have = (int(roster._speech[j, G.USER_NAME_LEN + 1] >> 1 & 1), int(roster._speech[j, 15]))
        if have != (int(bool(u["muzzled"])), u["muzzle"]):
            bad.append({"what": "muzzle mirror", "slot": j, "device": list(have), "want": [u["muzzled"], u["muzzle"]]})
    return bad


def seat_all(roster: G.Roster, users: dict) -> None:
    """go's seat, then the muzzles: the bit alone where the level byte stays 0, the level elsewhere."""
    seat(roster, users)
    ids = sorted(users)
    roster.update(ids, muzzle_level=[users[j]["muzzle"] for j in ids])
    bits = [j for j in ids if users[j]["muzzled"] and not users[j]["muzzle"]]
    if bits:
        roster.update(bits, muzzled=1)


# ------------------------------------------------------------------ seeded streams
def muzzle_some(rng: random.Random, users: dict) -> None:
    """A third of the users muzzled: half of them by the bit alone, the others at a level, the highest ones most often, so
    that an ``.unmuzzle`` meets a muzzle above its actor's level."""
    for u in users.values():
        kind = rng.random()
        u.setdefault("muzzle", 0)
        u.update(muzzled=int(kind < 0.35), muzzle=0 if kind >= 0.2 else rng.choice((WIZ, ARCH, G.MAX_LEVEL, G.MAX_LEVEL)))
        u["afk"] = u.get("afk") or int(rng.random() < 0.1)


def act_events(rng: random.Random, users: dict, rooms, k: int) -> list:
    """K events by actors of every level, the higher ones most often.  A fifth of the moves name a private room, so that a
    move refused as private is no rarity, and a fifth of the ``.unmuzzle`` events a user who is muzzled."""
    able = movers_of(users, len(rooms))
    high = sorted(able, key=lambda j: -users[j]["level"])[:max(1, len(able) // 3)]
    mid = [j for j in able if 1 <= users[j]["level"] < G.MAX_LEVEL]
    named = [rm["name"] for rm in rooms if rm["name"]] or [b"none"]
    private = [rm["name"] for rm in rooms if rm["name"] and rm["access"] & G.PRIVATE] or named
    people = [u["name"] for u in users.values() if u["name"]]
    muzzled = [u["name"] for u in users.values() if u["name"] and u["muzzled"]] or people
    events = []
    for _ in range(k):
        slot = rng.choice(high if rng.random() < 0.6 else able)
        com = rng.choice((G.COM_MOVE, G.COM_MOVE, G.COM_MOVE, G.COM_WAKE, G.COM_MUZZLE, G.COM_UNMUZZLE, G.COM_UNMUZZLE))
        kind = rng.random()
        word = (rng.choice(muzzled) if kind < 0.2 and com == G.COM_UNMUZZLE else rng.choice(people) if kind < 0.6
                else rng.choice(people).lower() if kind < 0.7 else rng.choice(people)[:-1] if kind < 0.78
                else users[slot]["name"] if kind < 0.84 else b"Nobody" if kind < 0.9 else b"n" * rng.choice((12, 13)) if kind < 0.93 else b"")
        room, kind = b"", rng.random()
        if com == G.COM_MOVE and word and kind < 0.15 and mid:             # by an actor who may lack the level, of a lower user
            slot = rng.choice(mid)
            lower = [u["name"] for u in users.values() if u["name"] and u["level"] < users[slot]["level"]]
            word = rng.choice(lower) if lower else word
        if com == G.COM_MOVE and word and kind < 0.75:
            room = (rng.choice(private) if kind < 0.15 else rng.choice(named) if kind < 0.55 else rng.choice(named)[:rng.randrange(1, 3)] if kind < 0.62
                    else rng.choice(named) + b"x" if kind < 0.68 else b"w" * rng.choice((20, 21, 45)))
        inpstr = rng.choice((b"", b" ", b"  ")) + word + (rng.choice((b" ", b"  ")) + room if room else b"") + rng.choice((b"", b"", b" \x01"))
        events.append((slot, com, inpstr, 1 if not word else 3 if room else 2))
    return events


def cases() -> list:
    caps, nrs = list(CAPACITIES), list(LOOK_ROOMS)
    return [(caps[i % len(caps)], nrs[i % len(nrs)]) for i in range(max(len(caps), len(nrs)) + 1)]


def following_differences(roster: G.Roster, users: dict, rooms, clones, rng: random.Random) -> list:
    """A go_many, an access_many, a look_many and a speak_many after the call: they see the moves and the muzzles only if
    the binding applied them and the mirrors went up again."""
    bad = []
    event = fuzz_events(rng, users, rooms, 1)
    call = go_call(users, rooms, clones, event, ARCH, 2)
    got = roster.go_many(event, gatecrash_level=ARCH, min_private_users=2)
    bad += [{"after": "go_many", **b} for b in go_differences(got, call, users, rooms)]
    event = access_events(rng, users, rooms, 1)
    call = access_call(users, rooms, clones, event, ARCH, 2, WIZ)
    got = roster.access_many(event, gatecrash_level=ARCH, min_private_users=2, ignore_mp_level=WIZ)
    bad += [{"after": "access_many", **b} for b in access_differences(got, call)]
    lookers = [j for j, u in users.items() if u["room"] is not None and u["room"] < len(rooms)][:8]
    if lookers:
        lk = roster.look_many(lookers)
        bad += [{"what": "look_many after", "slot": j} for i, j in enumerate(lookers) if lk.chunks(i) != look_of(users, rooms, j)]
    speakers = movers_of(users, len(rooms))[:8]
    said = roster.speak_many([(j, G.COM_SAY, b"hello", 2) for j in speakers])
    want = [G.MUZZLED if users[j]["muzzled"] else G.SPOKEN for j in speakers]
    if said.outcome.tolist() != want:
        bad.append({"what": "speak_many after", "device": said.outcome.tolist(), "want": want})
    return bad


def fuzz_part(seed: int, on_device: bool = True) -> dict:
    """Seeded streams over every capacity and room count; without ``on_device`` the model alone, for its outcomes."""
    rng = random.Random(seed)
    bad, outcomes, calls, events_n = [], {}, 0, 0
    for cap, nr in cases():
        rooms, users = fuzz_rooms(rng, nr), fuzz_users(rng, cap, nr)
        if not movers_of(users, nr):
            users[0].update(name=b"U0", login=0, room=0)
        muzzle_some(rng, users)
        clones = [(rng.randrange(cap), rng.randrange(nr), 2) if rng.random() < 0.5 else None for _ in range(3)]
        if on_device:
            roster = G.Roster(cap, look_rooms=nr, clones=len(clones), review_rooms=min(nr, 4))
            set_rooms(roster, rooms)
            seat_all(roster, users)
            seat_clones(roster, clones)
        for k in EVENTS + (1,):
            events = act_events(rng, users, rooms, k)
            gatecrash, min_private = rng.choice((0, 1, 2, 3, 4, 4)), rng.choice((0, 1, 2, 2, 3, 5, 2**31 - 1))
            call = act_call(users, rooms, clones, events, gatecrash, min_private)
            if on_device:
                got = roster.act_many(events, gatecrash_level=gatecrash, min_private_users=min_private)
                found = act_differences(got, call, users) + mirror_differences(roster, users, rooms) + muzzle_differences(roster, users)
                found += following_differences(roster, users, rooms, clones, rng)
                bad += [{"cap": cap, "look_rooms": nr, "k": k, **b} for b in found]
            calls += 1
            events_n += k
            for r in call["events"]:
                outcomes[r["outcome"]] = outcomes.get(r["outcome"], 0) + 1
        if on_device:
            roster.close()
    return {"cases": [list(c) for c in cases()], "events_per_call": list(EVENTS + (1,)), "calls": calls, "events": events_n,
            "outcomes": {str(k): v for k, v in sorted(outcomes.items())}, "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ get_user and get_room edges
GET_USER_WORDS = (b"anna", b"Anna", b"ann", b"abcdefghijkl", b"abcdefghijklm", b"bcdefghijkl", b"last", b"zan", b"Nna", b"host", b"prompt")


def edge_users() -> dict:
    """The access child's names at the edges, with a GOD for an actor: an exact match at slot 64 behind a substring match
    at slot 63; a login slot below both that holds the exact name; a 12-byte name."""
    return {0: act_user(0, name=b"Zanna", room=1), 63: act_user(63, name=b"Annabel", room=1), 64: act_user(64, name=b"Anna", room=1),
            255: act_user(255, name=b"Abcdefghijkl", room=1), 256: act_user(256, name=b"Last", room=1),
            10: act_user(10, name=b"Anna", room=1, login=1), 11: act_user(11, name=None, room=1),
            5: act_user(5, name=b"Host", room=0, level=G.MAX_LEVEL), 6: act_user(6, name=b"Prompt", room=1, login=1)}


def get_user_part() -> dict:
    """Every word as ``.wake <word>``, ``.muzzle <word>`` and ``.move <word>`` by the GOD in the other room, a call each."""
    rooms = [list_room(b"den", links=[1]), list_room(b"hall", links=[0])]
    users = edge_users()
    roster = G.Roster(257, look_rooms=2)
    set_rooms(roster, rooms)
    seat_all(roster, users)
    targets, bad = [], []
    for com in (G.COM_WAKE, G.COM_MUZZLE, G.COM_MOVE):
        for w in GET_USER_WORDS:
            events = [(5, com, w, 2)]
            call = act_call(users, rooms, [], events, ARCH, 2)
            got = roster.act_many(events, gatecrash_level=ARCH, min_private_users=2)
            targets.append([int(got.outcome[0]), int(got.target_slot[0])])
            bad += [{"word": w.decode(), "com": com, **b}
                    for b in act_differences(got, call, users) + mirror_differences(roster, users, rooms) + muzzle_differences(roster, users)]
    roster.close()
    return {"targets": targets, "n_bad": len(bad), "first_bad": bad[:2]}


def get_room_part() -> dict:
    """The words of the go child's get_room_part as ``word[2]`` of ``.move guest <word>``, typed by an ARCH; the target is
    put back between the calls."""
    out, bad = {}, []
    for label, nr, twins in (("255_256", 300, (255, 256)), ("0_1023", 1024, (0, 1023))):
        rooms = [list_room(b"n%d" % i, links=[]) for i in range(nr)]
        rooms[twins[0]]["name"], rooms[twins[1]]["name"] = b"twinroom_a", b"twinroom_b"
        rooms[3]["name"] = b"exactly_twenty_bytes"
        rooms[7]["name"] = b""                                          # a nameless room in between
        users = {0: act_user(0, name=b"Arch", room=5, level=ARCH), 1: act_user(1, name=b"Guest", room=6)}
        roster = G.Roster(2, look_rooms=nr)
        set_rooms(roster, rooms)
        seat_all(roster, users)
        words = (b"twin", b"twinroom_b", b"twinroom_", b"exactly_twenty_bytes", b"exactly_twenty_bytesx", b"exactly_twenty_byte",
                 b"n7", b"n%d" % (nr - 1), b"twinroom_c")
        got_targets = []
        for w in words:
            events = [(0, G.COM_MOVE, b"guest " + w, 3)]
            call = act_call(users, rooms, [], events, ARCH, 2)
            got = roster.act_many(events, gatecrash_level=ARCH, min_private_users=2)
            got_targets.append(int(got.target_room[0]))
            bad += [{"part": label, "word": w.decode(), **b} for b in act_differences(got, call, users) + mirror_differences(roster, users, rooms)]
            users[1]["room"] = 6
            roster.update(1, room=6)
        out[label] = got_targets
        roster.close()
    return {"targets": out, "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ repeatability, regrowth, limits
def digest(got: G.Act) -> str:
    return digest_of(got, [got.target_slot, got.target_room, got.old_room, got.returned_public], texts_of(got))


def fuzz_state(rng: random.Random, cap: int, nr: int):
    rooms, users = fuzz_rooms(rng, nr), fuzz_users(rng, cap, nr)
    muzzle_some(rng, users)
    return rooms, users


def determinism_part(seed: int) -> dict:
    runs = []
    for _ in range(2):
        rng = random.Random(seed)
        rooms, users = fuzz_state(rng, 257, 6)
        roster = G.Roster(257, look_rooms=6)
        set_rooms(roster, rooms)
        seat_all(roster, users)
        events = act_events(rng, users, rooms, 64)
        kw = {"gatecrash_level": ARCH, "min_private_users": 2}
        first = digest(roster.act_many(events, **kw))
        seat_all(roster, users)                                         # back to the rooms, the muzzles and the access before
        set_rooms(roster, rooms)
        runs.append([first, digest(roster.act_many(events, **kw))])
        roster.close()
    return {"same_on_a_second_call": runs[0][0] == runs[0][1], "same_on_a_second_roster": runs[0] == runs[1]}


def regrown_part(seed: int) -> dict:
    """A small call that changes nothing, then one large enough to make the roster's device allocation grow: the table is
    not dirty, and has to travel again from the pinned mirror."""
    rng = random.Random(seed)
    cap, nr = 65, 6
    rooms, users = fuzz_state(rng, cap, nr)
    roster = G.Roster(cap, look_rooms=nr)
    set_rooms(roster, rooms)
    seat_all(roster, users)
    actor = movers_of(users, nr)[0]
    kw = {"gatecrash_level": ARCH, "min_private_users": 2}
    small = roster.act_many([(actor, G.COM_WAKE, b"", 1)], **kw)
    clean = not (roster._dirty or roster._go_dirty or roster._rooms_dirty or roster._speech_dirty)
    events = act_events(rng, users, rooms, 600)
    call = act_call(users, rooms, [], events, ARCH, 2)
    big = roster.act_many(events, **kw)
    bad = act_differences(big, call, users) + mirror_differences(roster, users, rooms) + muzzle_differences(roster, users)
    bad += following_differences(roster, users, rooms, [], rng)
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
    room[cap - 400:] = 500                                              # the far end of the table stands in one room nobody enters
    ids = list(range(cap))
    level = [G.MAX_LEVEL if j < 32 and j % 2 == 0 else 1 for j in ids]  # the first of each pair is a GOD
    users = {j: act_user(j, name=b"U%d" % j, room=int(room[j]), level=level[j], colour=j & 1) for j in ids}
    roster = G.Roster(cap, look_rooms=nr, clones=G.MAX_CAPACITY)
    set_rooms(roster, rooms)
    roster.update(ids, room=room.tolist(), name=[b"U%d" % j for j in ids], level=level, colour=[j & 1 for j in ids])
    crooms = np.full(G.MAX_CAPACITY, 9, dtype=np.int32)
    crooms[-1] = 12                                                     # the last record stands in the private room 12
    roster.set_clones(list(range(G.MAX_CAPACITY)), owner=20, room=crooms.tolist())
    clones = [(20, int(r), G.CLONE_HEAR_ALL) for r in crooms]
    far = lambda base, i: b"u%d" % (cap - base - i)
    muzzled = [cap - 200 - i for i in range(8)]                         # muzzled by a WIZ before the call
    for j in muzzled:
        users[j].update(muzzled=1, muzzle=WIZ)
    roster.update(muzzled, muzzle_level=WIZ)
    # the GODs of the rooms 8 .. 15 move their room-mates to the far end (out of the private rooms 10 .. 15, which return to
    # public but room 12, where the last clone stands); those of the rooms 0 .. 7 muzzle, wake and unmuzzle users at the far
    # end of the table, and are woken by their room-mates; then a refusal of every command
    events = [(2 * i, G.COM_MOVE, b"u%d room%04d" % (2 * i + 1, nr - 1 - i), 3) for i in range(8, 16)]
    events += [(2 * i, G.COM_MUZZLE, far(1, i), 2) for i in range(8)]
    events += [(2 * i, G.COM_WAKE, far(100, i), 2) for i in range(8)]
    events += [(2 * i, G.COM_UNMUZZLE, far(200, i), 2) for i in range(8)]
    events += [(2 * i + 1, G.COM_WAKE, b"u%d" % (2 * i), 2) for i in range(8)]
    events += [(2 * i, G.COM_MOVE, b"u%d" % (2 * i), 2) for i in range(8)]
    events += [(2 * i, G.COM_MUZZLE, b"nobodyhere", 2) for i in range(8)]
    events += [(2 * i, G.COM_UNMUZZLE, far(300, i), 2) for i in range(k - len(events))]
    call = act_call(users, rooms, clones, events, ARCH, 2)
    t0 = time.perf_counter()
    got = roster.act_many(events, gatecrash_level=ARCH, min_private_users=2)
    seconds = time.perf_counter() - t0
    bad = act_differences(got, call, users)
    want_room = np.array([users[j]["room"] for j in ids], dtype=np.int32)
    mirror_ok = bool((roster._room == want_room).all()) and [int(roster._room_rec[r, 21]) for r in range(nr)] == [rm["access"] for rm in rooms]
    muzzled = int((roster._speech[:, 15] != 0).sum())
    privates = [r for r in range(16) if int(roster._room_rec[r, 21]) == G.PRIVATE]
    roster.close()
    return {"capacity": cap, "look_rooms": nr, "clones": G.MAX_CAPACITY, "k": len(events), "seconds": round(seconds, 3),
            "outcomes": sorted(set(got.outcome.tolist())), "mirror_ok": mirror_ok, "privates": privates, "muzzled": muzzled,
            "want_muzzled": sum(1 for u in users.values() if u["muzzle"]), "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ the recorded sessions
SESSIONS = ("reference_only/act.json", "reference_only/clone.json", "reference_only/replay_8.json")
ABSENT = (G.ACT_MUZZLE_ABSENT, G.ACT_UNMUZZLE_ABSENT)


class ActState(sr.State):
    """The replayer's state with ``muzzle``, the level of a user's muzzle: an account provisioned muzzled has the bit alone."""

    def __init__(self, doc: dict, layout: str):
        super().__init__(doc, layout)
        cfg = doc["config"]                                             # a session recorded with settings of its own says so
        self.gatecrash, self.min_private = int(cfg.get("gatecrash_level", self.gatecrash)), int(cfg.get("min_private", self.min_private))
        self.ignore_mp = int(cfg.get("ignore_mp_level", self.ignore_mp))

    def login(self, actor: str, name: str) -> None:
        super().login(actor, name)
        self.users[self.seats[actor]]["muzzle"] = 0

    def everyone(self) -> dict:
        out = super().everyone()
        for u in out.values():
            u.setdefault("muzzle", 0)
        return out


class ActModelBackend(sr.ModelBackend):
    def afk(self, slot: int, on: int) -> None:
        """The state has the flag; ``sync`` gives it to the model."""

    def act(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        """One event through the model.  It changes ``self.all`` and the state's rooms as the event does."""
        st = self.st
        call = act_call(self.all, st.rooms, st.table(), [(slot, com, inpstr, word_count)], st.gatecrash, st.min_private)
        res = call["events"][0]
        for rm in call["cleared"]:
            self.rings.clear(rm)
        return self._answer(res, KINDS, room=res["room"], target_room=res["target_room"], target_slot=res["target_slot"], old=res["old"],
                            returned=res["returned"], look=b"".join(res["look"]) if res["outcome"] in MOVED else None)


class ActDeviceBackend(sr.DeviceBackend):
    """One roster for the session.  After an ``act_many`` the replayer's state takes the event's changes from what the call
    returned; nothing of them is uploaded, and the roster's mirrors -- the muzzles among them -- are compared with it."""

    def act(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        st = self.st
        got = self.roster.act_many([(slot, com, inpstr, word_count)], gatecrash_level=st.gatecrash, min_private_users=st.min_private)
        self._count("act_many")
        a = self._answer(got, texts_of(got), room=st.users[slot]["room"], target_room=int(got.target_room[0]),
                         target_slot=int(got.target_slot[0]), old=int(got.old_room[0]), returned=bool(got.returned_public[0]))
        if a["outcome"] in EFFECTIVE:
            apply_act(st.users, st.rooms, {"slot": slot, "outcome": a["outcome"], "target_slot": a["target_slot"],
                                           "target_room": a["target_room"], "old": a["old"], "returned": a["returned"], "look": None}, [])
        if a["outcome"] in MOVED:
            a["look"] = got.look.output(0)
        return a

    def afk(self, slot: int, on: int) -> None:
        """``.afk`` and the return from it are not answered here: the roster is told the flag."""
        self._upload("update", slot, afk=on)

    def mirror(self) -> list:
        return super().mirror() + muzzle_differences(self.roster, self.st.users)


class ActReplayer(sr.Replayer):
    """``sr.Replayer`` with ``.move``, ``.wake``, ``.muzzle`` and ``.unmuzzle`` answered: the outcome and the texts come from
    the backend's ``act``, nothing of them from the recording, and every client's bytes are compared, the actor's included.
    The four room lines reach the clones' owners through ``relay_many``, and the moved user's prompt is composed here.  The
    two ``*_ABSENT`` branches read the user file: their bytes are the caller's, and taken from the recording.  The commands
    of STATE_ONLY change the state and are answered by nobody here, as in ``GoReplayer``: an ``.afk`` sets the flag, in the
    state and on the roster, and the next input of that user ends it (c:176-187) and is not run."""
    STATE_ONLY = ("afk", "myclones", "switch", "write")

    def __init__(self, doc: dict, backend_class=ActModelBackend, layout: str = sr.COMPACT):
        self._begin(doc, ActState(doc, layout), backend_class)
        self.res.update(act=0, act_outcomes={}, act_lines=0, state_only=0)

    def _line_of(self, out: dict, a: dict, kind: str, rm: int, sender, com: int, same_plan: bool = True) -> None:
        """A room line the call composed and planned, delivered by the call's plan and relay_many's relays.  relay_many sees
        the roster as the call left it: its plan of the line is the call's unless the moved user stands among the listeners
        before the move and not after it, or the other way round (the here line)."""
        text = a["texts"][kind]
        if text is None:
            return
        part = self.backend.relay([(text, rm, sender, 0, com)])[0]
        if same_plan:
            self.res["plan_checks"] += 1
            self.res["plan_disagreements"] += part["plan"] != a["plans"][kind]
        self._deliver(out, [{"plan": a["plans"][kind], "relays": part["relays"]}])

    def _answer(self, index: int, step: dict, u: dict, inp: dict, what: str) -> None:
        st, slot, com = self.st, u["slot"], inp["com"]
        out = {j: b"" for j in st.users}
        in_ring = None
        a = self.backend.act(slot, com, inp["inpstr"], inp["word_count"])
        self.res["act"] += 1
        self.res["act_outcomes"][a["outcome"]] = self.res["act_outcomes"].get(a["outcome"], 0) + 1
        if a["outcome"] == G.ACT_DEFERRED:
            self.res["mismatches"].append({"step": index, "send": step["send"][:80], "what": "a call of one event deferred"})
        if a["outcome"] in ABSENT:                                      # the caller's branch: the user file
            out[slot] += step["recv"].get(step["actor"], "").encode("latin-1")
        who = a["target_slot"]
        if a["texts"]["reply"] is not None:
            out[slot] += b"".join(a["plans"]["reply"]["chunks"][u["colour"]])
        self._line_of(out, a, "here", a["room"], slot, com, same_plan=False)
        if a["texts"]["notice"] is not None:
            out[who] += b"".join(a["plans"]["notice"]["chunks"][st.users[who]["colour"]])
        # move_user writes the enter line before it moves the user; the roster has moved it, so the target is the sender
        self._line_of(out, a, "enter", a["target_room"], who, com)
        self._line_of(out, a, "leave", a["old"], who, com)
        if a["look"] is not None:
            out[who] += a["look"]
        if a["returned"]:
            self._returned_to_public(index, step, a["old"])
        self._line_of(out, a, "reset", a["old"], who, com)
        if a["look"] is not None and st.users[who]["command_mode"]:     # prompt(u), c:4767
            out[who] += nuts_path.transduce(b"~FTCOM> " if st.users[who]["vis"] else b"~FTCOM+> ", st.users[who]["colour"])
        if u["command_mode"] and a["outcome"] not in ABSENT:
            out[slot] += nuts_path.transduce(b"~FTCOM> " if u["vis"] else b"~FTCOM+> ", u["colour"])
        self.res["commands"][what] = self.res["commands"].get(what, 0) + 1
        self.res["answered"] += 1
        for actor, j in st.seats.items():
            got, want = out[j], step["recv"].get(actor, "").encode("latin-1")
            self.res["comparisons"] += 1
            if got != want:
                self.res["mismatches"].append({"step": index, "send": step["send"][:80], "by": step["actor"], "client": actor,
                                               "got": got.decode("latin-1")[:400], "want": want.decode("latin-1")[:400]})
        self.res["mirror_checks"] += 1
        for m in self.backend.mirror():
            self.res["mismatches"].append({"step": index, "send": step["send"][:80], "by": step["actor"], **m})

    def line(self, index: int, step: dict) -> None:
        st = self.st
        u = st.users[st.seats[step["actor"]]]
        if u.get("afk"):                                                # any input ends AFK (c:176-187): the line is not run
            u["afk"] = 0
            self.backend.afk(u["slot"], 0)
            self.res["state_only"] += 1
            return
        if (step["send"].split() or [""])[0].lstrip(".") in COMS:
            self.res["act_lines"] += 1
        self.backend.sync()
        inp = self.backend.input(u["slot"], step["send"].encode("latin-1") + b"\n", record=False)
        what = nuts_path.lib().np_command_name(inp["com"]).decode() if inp["kind"] == sr.COMMAND else None
        if what in COMS:
            self._answer(index, step, u, inp, what)
            return
        if what in self.STATE_ONLY:
            if what == "afk":
                u["afk"] = 1
                self.backend.afk(u["slot"], 1)
            elif what == "switch" and "strange sensation" in step["recv"].get(step["actor"], ""):   # clone_switch, c:7263-7290
                i = st.find_clone(u["slot"], st.get_room(sr.words_of(inp["inpstr"])[0]))
                st.clones[i][1], u["room"] = u["room"], st.clones[i][1]
            self.res["state_only"] += 1
            return
        super().line(index, step)


def act_lines(doc: dict) -> int:
    return lines_of(doc, COMS)


def replay_sessions(backend_class=ActModelBackend, layouts=(sr.COMPACT,)) -> dict:
    out = {}
    for name in SESSIONS:
        doc = load(name)
        for layout in layouts:
            if layout == sr.SPREAD and len(doc["accounts"][0]) not in sr.SPREAD_SLOTS:
                continue
            res = ActReplayer(doc, backend_class, layout).run()
            out[f"{name}:{layout}"] = {"act": res["act"], "act_lines": act_lines(doc), "answered": res["answered"], "state_only": res["state_only"],
                                      "outcomes": {str(k): v for k, v in sorted(res["act_outcomes"].items())},
                                      "comparisons": res["comparisons"], "mismatches": res["mismatches"][:2],
                                      "n_mismatches": len(res["mismatches"]), "capacity": res["capacity"],
                                      "plan_disagreements": res["plan_disagreements"], "calls": res["calls"].get("act_many", 0)}
    return out


def parts(seed: int) -> tuple:
    return (("golden", lambda: replay_sessions(ActDeviceBackend, (sr.COMPACT, sr.SPREAD))), ("fuzz", lambda: fuzz_part(seed)),
            ("get_user", get_user_part), ("get_room", get_room_part),
            ("determinism", lambda: determinism_part(seed + 1)), ("regrown", lambda: regrown_part(seed + 2)), ("limits", limits_part))


def profile(res: dict) -> dict:
    return {"seconds": res["seconds"], "fuzz": {k: res["fuzz"][k] for k in ("calls", "events", "outcomes")},
            "golden": {k: {"act": v["act"], "comparisons": v["comparisons"]} for k, v in res["golden"].items()},
            "limits_seconds": res["limits"]["seconds"]}


def main() -> int:
    return child_main("DEVICE_ACT", parts, profile, seed=20263)


if __name__ == "__main__":
    sys.exit(main())
