"""The device work of tests/test_device_set.py, in a short-lived child process of its own, and the CPU model the host tier
of that module shares with it.

As tests/device_access_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_SET {...}``).  ``setting`` is the Python model of ``toggle_mode``, ``toggle_ignall``,
``toggle_prompt``, ``set_desc``, ``set_iophrase``, ``set_topic``, ``visibility``, ``toggle_charecho``, ``afk``,
``toggle_colour``, ``toggle_ignshout`` and ``toggle_igntell`` (nuts333.c:4009-4018, 4463-4539, 4697-4722, 6434-6455,
6881-6893, 7409-7507), built from the reference's format strings; ``set_call`` is the model of one ``Roster.set_many``
call: it runs the events ONE AFTER ANOTHER, each against the state the earlier ones left, and defers by the rule of the
call -- so a device that decides every event against the snapshot agrees with it only if the rule makes the two the same.
``SetReplayer`` answers these steps of the recorded sessions through a backend's ``set`` method and compares every
client's bytes, the actor's included; what ``user_input`` does for a user who is AFK (nuts333.c:180-203) is the caller's,
and the replayer composes it from the format strings.

    python tests/device_set_child.py [--seed S]
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
from device_go_child import admitted, first_word, go_call, go_differences, go_user, look_of  # noqa: E402
from device_go_child import set_rooms as set_list_rooms  # noqa: E402
from device_rooms_child import list_room  # noqa: E402
from device_rooms_child import model_chunks as rooms_chunks  # noqa: E402
from device_tell_child import private  # noqa: E402
from device_who_child import model_chunks as who_chunks  # noqa: E402
from event_checks import child_main, event_differences, plan_of  # noqa: E402
from event_checks import digest as digest_of  # noqa: E402
from event_checks import load as load_golden  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402

G = device
NAMES = {"mode": G.COM_MODE, "ignall": G.COM_IGNALL, "prompt": G.COM_PROMPT, "desc": G.COM_DESC, "inphr": G.COM_INPHR,
         "outphr": G.COM_OUTPHR, "topic": G.COM_TOPIC, "vis": G.COM_VIS, "invis": G.COM_INVIS, "charecho": G.COM_CHARECHO,
         "afk": G.COM_AFK, "colour": G.COM_COLOUR, "ignshout": G.COM_IGNSHOUT, "igntell": G.COM_IGNTELL}
#: the steps sr.Replayer tracks from format strings and SetReplayer answers
WAS_TRACKED = ("colour", "ignall", "ignshout", "igntell", "vis", "invis")
KINDS = ("here", "reply", "reply2")
EFFECTIVE = tuple(range(G.SET_IGNTELL_OFF + 1))
HEARD = (G.SET_IGNALL_ON, G.SET_IGNALL_OFF, G.SET_COLOUR_ON, G.SET_COLOUR_OFF)
CAPACITIES, EVENTS, EDGE_SLOTS = (1, 8, 63, 64, 65, 257), (1, 3, 4, 5, 64, 65), (0, 63, 64, 256)
PASSWORD = b"test"                                                      # every provisioned account's


# ------------------------------------------------------------------ the model
def set_user(slot: int, **fields) -> dict:
    return go_user(slot, **{"charmode_echo": 0, "last_login": 0, "away": None, **fields})


def toggle(u: dict, field: str, on, off, said_on: bytes, said_off: bytes):
    """A toggle that reports what it found: (outcome, reply, change)."""
    return (off, said_off, {field: 0}) if u[field] else (on, said_on, {field: 1})


def setting(users: dict, rooms, slot: int, com: int, inpstr: bytes, wc: int) -> dict:
    """What one such command does, without doing it: the outcome, the three texts, the colour the replies are written
    with, and what it changes: ``change`` of the user's fields (``afk`` is 2 for a locked session) and ``topic``."""
    u = users[slot]
    res = {"slot": slot, "com": com, "outcome": None, "room": u["room"], "here": None, "reply": None, "reply2": None, "change": {},
           "topic": None, "reply_colour": u["colour"]}
    me, word = u["name"], first_word(inpstr)

    def done(outcome, reply, **more):
        res.update(outcome=outcome, reply=reply, **more)
        return res

    if com == G.COM_MODE:                                               # toggle_mode, c:4012-4017
        o, r, c = toggle(u, "command_mode", G.SET_MODE_COMMAND, G.SET_MODE_SPEECH, b"Now in COMMAND mode.\n", b"Now in SPEECH mode.\n")
        return done(o, r, change=c)
    if com == G.COM_IGNALL:                                             # toggle_ignall, c:4466-4476: user->name
        if not u["ignall"]:
            return done(G.SET_IGNALL_ON, b"You are now ignoring everyone.\n", here=b"%s is now ignoring everyone.\n" % me, change={"ignall": 1})
        return done(G.SET_IGNALL_OFF, b"You will now hear everyone again.\n", here=b"%s is listening again.\n" % me, change={"ignall": 0})
    if com == G.COM_PROMPT:                                             # toggle_prompt, c:4484-4489
        o, r, c = toggle(u, "prompt", G.SET_PROMPT_ON, G.SET_PROMPT_OFF, b"Prompt ~FGON.\n", b"Prompt ~FROFF.\n")
        return done(o, r, change=c)
    if com == G.COM_CHARECHO:                                           # toggle_charecho, c:6884-6891
        o, r, c = toggle(u, "charmode_echo", G.SET_CHARECHO_ON, G.SET_CHARECHO_OFF, b"Echoing for character mode clients ~FGON.\n",
                         b"Echoing for character mode clients ~FROFF.\n")
        return done(o, r, change=c)
    if com == G.COM_IGNSHOUT:                                           # toggle_ignshout, c:7487-7493
        o, r, c = toggle(u, "ignshout", G.SET_IGNSHOUT_ON, G.SET_IGNSHOUT_OFF, b"You are now ignoring shouts and shout emotes.\n",
                         b"You are no longer ignoring shouts and shout emotes.\n")
        return done(o, r, change=c)
    if com == G.COM_IGNTELL:                                            # toggle_igntell, c:7500-7506
        o, r, c = toggle(u, "igntell", G.SET_IGNTELL_ON, G.SET_IGNTELL_OFF, b"You are now ignoring tells and private emotes.\n",
                         b"You are no longer ignoring tells and private emotes.\n")
        return done(o, r, change=c)
    if com == G.COM_VIS:                                                # visibility(user, 1), c:6439-6446
        if u["vis"]:
            return done(G.SET_ALREADY_VISIBLE, b"You are already visible.\n")
        return done(G.SET_VISIBLE, b"~FB~OLYou recite a melodic incantation and reappear.\n",
                    here=b"~FB~OLYou hear a melodic incantation chanted and %s materialises!\n" % me, change={"vis": 1})
    if com == G.COM_INVIS:                                              # visibility(user, 0), c:6448-6454
        if not u["vis"]:
            return done(G.SET_ALREADY_INVISIBLE, b"You are already invisible.\n")
        return done(G.SET_INVISIBLE, b"~FB~OLYou recite a melodic incantation and fade out.\n",
                    here=b"~FB~OL%s recites a melodic incantation and disappears!\n" % me, change={"vis": 0})
    if com == G.COM_COLOUR:                                             # toggle_colour, c:7465-7479
        if u["command_mode"] and u["ignall"] and u["charmode_echo"]:
            return done(G.SET_COLOUR_TEST, None)
        if u["colour"]:                                                 # written, then cleared; set, then written
            return done(G.SET_COLOUR_OFF, b"Colour ~FROFF.\n", change={"colour": 0}, reply_colour=1)
        return done(G.SET_COLOUR_ON, b"Colour ~FGON.\n", change={"colour": 1}, reply_colour=1)
    if com == G.COM_DESC:                                               # set_desc, c:4498-4510
        if wc < 2:
            return done(G.SET_DESC_QUERY, b"Your current description is: %s\n" % u["desc"])
        if b"(CLONE)" in word:
            return done(G.SET_DESC_CLONE, b"You cannot have that description.\n")
        if len(inpstr) > G.USER_DESC_LEN:
            return done(G.SET_DESC_LONG, b"Description too long.\n")
        return done(G.SET_DESC_SET, b"Description set.\n", change={"desc": inpstr})
    if com in (G.COM_INPHR, G.COM_OUTPHR):                              # set_iophrase, c:4519-4538
        if len(inpstr) > G.PHRASE_LEN:
            return done(G.SET_PHRASE_LONG, b"Phrase too long.\n")
        which, field, asked, is_set = ((b"in", "in_phrase", G.SET_INPHR_QUERY, G.SET_INPHR_SET) if com == G.COM_INPHR
                                       else (b"out", "out_phrase", G.SET_OUTPHR_QUERY, G.SET_OUTPHR_SET))
        if wc < 2:
            return done(asked, b"Your current %s phrase is: %s\n" % (which, u[field]))
        return done(is_set, b"%s phrase set.\n" % which.capitalize(), change={field: inpstr})
    if com == G.COM_TOPIC:                                              # set_topic, c:4705-4721
        topic = rooms[u["room"]]["topic"]
        if wc < 2:
            if not topic:
                return done(G.SET_TOPIC_NONE, b"No topic has been set yet.\n")
            return done(G.SET_TOPIC_QUERY, b"The current topic is: %s\n" % topic)
        if len(inpstr) > G.TOPIC_LEN:
            return done(G.SET_TOPIC_LONG, b"Topic too long.\n")
        shown = me if u["vis"] else G.INVISNAME
        return done(G.SET_TOPIC_SET, b"Topic set to: %s\n" % inpstr, here=b"%s has set the topic to: %s\n" % (shown, inpstr), topic=inpstr)
    assert com == G.COM_AFK                                             # afk, c:7413-7453
    outcome, reply, mesg = G.SET_AFK, b"You are now AFK, press <return> to reset.\n", b""
    if wc > 1:
        mesg = inpstr
        if word == b"lock":
            outcome, reply = G.SET_AFK_LOCKED, b"You are now AFK with the session locked, enter your password to unlock it.\n"
            mesg = G._remove_first(inpstr)
        if len(mesg) > G.AFK_MESG_LEN:
            return done(G.SET_AFK_LONG, b"AFK message too long.\n")
    change = {"afk": 2 if outcome == G.SET_AFK_LOCKED else 1}
    if mesg:
        change["afk_mesg"] = mesg
        res["reply2"] = b"AFK message set.\n"
    kept = mesg or u["afk_mesg"]
    if u["vis"]:
        res["here"] = b"%s goes AFK: %s\n" % (me, kept) if kept else b"%s goes AFK...\n" % me
    return done(outcome, reply, change=change)


def apply_set(users: dict, rooms, res: dict) -> None:
    users[res["slot"]].update(res["change"])
    if res["topic"] is not None:
        rooms[res["room"]]["topic"] = res["topic"]


def set_call(users: dict, rooms, events) -> dict:
    """One set_many call: the events one after another on ``users`` and ``rooms``, which it changes.  An event is deferred
    when an earlier effective event of the call that was not deferred had its actor; or toggled ``ignall`` or ``colour`` in
    its actor's room, and it has a here line; or set the topic of its actor's room, and it is a ``.topic``."""
    actors, heard, topics, out = set(), set(), set(), []
    for slot, com, inpstr, wc in events:
        res = setting(users, rooms, slot, com, inpstr, wc)
        if slot in actors or (res["here"] is not None and res["room"] in heard) or (com == G.COM_TOPIC and res["room"] in topics):
            res.update(outcome=G.SET_DEFERRED, here=None, reply=None, reply2=None, change={}, topic=None)
        res["plans"] = {"here": admitted(users, res["room"], slot) if res["here"] is not None else [],
                        "reply": [slot] if res["reply"] is not None else [], "reply2": [slot] if res["reply2"] is not None else []}
        if res["outcome"] in EFFECTIVE:
            actors.add(slot)
            if res["outcome"] in HEARD:
                heard.add(res["room"])
            if res["outcome"] == G.SET_TOPIC_SET:
                topics.add(res["room"])
            apply_set(users, rooms, res)
        out.append(res)
    return {"events": out}


def texts_of(got: G.Settings):
    return (("here", got.here, got.here_text), ("reply", got.reply, got.reply_text), ("reply2", got.reply2, got.reply2_text))


def set_differences(got: G.Settings, call: dict) -> list:
    """Everything a Settings says against the model's call."""
    return event_differences(got, call, texts_of(got), G.SET_DEFERRED, lambda k, res: ((int(got.reply_colour[k]),), (res["reply_colour"],)),
                             effective=EFFECTIVE)


def deliveries(users_before: dict, call: dict) -> dict:
    """What every slot receives of a set_call, per client: the events in call order, and of one event the reply, the second
    reply, the here line; SET_COLOUR_TEST is the caller's twenty lines.  ``users_before`` holds the colours before it."""
    colour = {j: u["colour"] for j, u in users_before.items()}
    out = {j: b"" for j in users_before}
    for res in call["events"]:
        slot = res["slot"]
        if res["outcome"] == G.SET_COLOUR_TEST:
            out[slot] += b"".join(nuts_path.transduce(line, colour[slot]) for line in G.COLOUR_TEST)
        for kind in ("reply", "reply2"):
            if res[kind] is not None:
                out[slot] += b"".join(nuts_path.chunks(res[kind], res["reply_colour"]))
        for j in res["plans"]["here"]:
            out[j] += b"".join(nuts_path.chunks(res["here"], colour[j]))
        colour[slot] = res["change"].get("colour", colour[slot])
    return out


# ------------------------------------------------------------------ a roster and its model
FLAG_FIELDS = ("login", "ignall", "ignshout", "colour")
SPEECH_FIELDS = ("vis", "muzzled", "command_mode", "igntell", "prompt", "charmode_echo")


def seat(roster: G.Roster, users: dict) -> None:
    ids = sorted(users)
    named = [j for j in ids if users[j]["name"]]
    if named:
        roster.update(named, name=[users[j]["name"] for j in named])
    for f in ("room",) + FLAG_FIELDS + SPEECH_FIELDS + ("level", "afk_mesg", "desc", "in_phrase", "out_phrase", "last_login"):
        roster.update(ids, **{f: [users[j][f] for j in ids]})
    roster.update(ids, afk=[int(bool(users[j]["afk"])) for j in ids])


def mirror_differences(roster: G.Roster, users: dict, rooms) -> list:
    """The roster's host mirrors against the model's state."""
    bad = []
    text = lambda row, n: bytes(row[:row[n]])
    for j, u in users.items():
        have = {f: int(bool(roster._flags[j] & G.ROSTER_FLAGS[f])) for f in FLAG_FIELDS}
        have.update({f: int(bool(roster._speech[j, G.USER_NAME_LEN + 1] & {**G.SPEECH_FLAGS, **G.SET_FLAGS}[f])) for f in SPEECH_FIELDS + ("afk",)})
        have.update(desc=text(roster._udesc[j], G.USER_DESC_LEN), afk_mesg=text(roster._afk[j], G.AFK_MESG_LEN),
                    in_phrase=text(roster._go[j], G.PHRASE_LEN), out_phrase=text(roster._go[j, G._GO_OUT:], G.PHRASE_LEN))
        want = {f: (int(bool(u[f])) if f == "afk" else u[f]) for f in have}
        if have != want:
            bad.append({"what": "user mirror", "slot": j, "fields": sorted(f for f in have if have[f] != want[f])})
    for r, rm in enumerate(rooms[:roster.look_rooms]):
        if bytes(roster._room_rec[r, 72:72 + roster._room_rec[r, 23]]) != rm["topic"]:
            bad.append({"what": "topic mirror", "room": r})
    return bad


WORDS = (b"", b"x", b"lock", b"lock ", b"lockx", b"Lock", b"a(CLONE)b", b"(CLONE)", b"(CLONE", b"~FRred~RS", b"\xe9\xff", b"gone /~fishing")


def fuzz_state(rng: random.Random, cap: int, nr: int):
    """``nr`` look rooms and ``cap`` slots: users at the edge slots and at random ones, in the look rooms or, one in five, in
    room ``nr`` + 1, which has no record; both colours, every flag, kept descriptions, phrases and AFK messages."""
    rooms = [list_room(b"room%d" % i, links=[], topic=(b"", b"a ~FGtopic", b"t" * 60)[(i + cap) % 3]) for i in range(nr)]
    slots = sorted({j for j in EDGE_SLOTS if j < cap} | set(rng.sample(range(cap), min(cap, 12))))
    users = {}
    for j in range(cap):
        bit = lambda p=0.3: int(rng.random() < p)
        users[j] = set_user(j, name=(b"U%d" % j if j % 7 else b"Twelve_%05d" % j) if j in slots else None,
                            room=nr + 1 if bit(0.2) else rng.randrange(min(nr, 3)), colour=bit(0.5), vis=bit(0.8), level=rng.randrange(5),
                            ignall=bit(), ignshout=bit(), igntell=bit(), command_mode=bit(), prompt=bit(), charmode_echo=bit(),
                            login=int(j not in slots and bit(0.1)), desc=rng.choice((b"", b"is a bot", b"d" * 30, b"~FR/desc")),
                            afk_mesg=rng.choice((b"", b"", b"brb", b"m" * 60)), in_phrase=rng.choice((b"enters", b"", b"p" * 40)),
                            out_phrase=rng.choice((b"goes", b"o" * 40)))
    return rooms, users, slots


def fuzz_events(rng: random.Random, users: dict, rooms, actors, k: int) -> list:
    events = []
    limit = {G.COM_DESC: G.USER_DESC_LEN, G.COM_INPHR: G.PHRASE_LEN, G.COM_OUTPHR: G.PHRASE_LEN, G.COM_TOPIC: G.TOPIC_LEN, G.COM_AFK: G.AFK_MESG_LEN}
    for _ in range(k):
        slot = rng.choice(actors)
        coms = [c for c in G.SET_COMS if c != G.COM_TOPIC or users[slot]["room"] < len(rooms)]
        com = rng.choice(coms)
        kind = rng.random()
        if com not in limit or kind < 0.25:
            inpstr = rng.choice((b"", b"", b"ignored words"))
        elif kind < 0.45:                                               # at the limit and one past it
            n = limit[com] + rng.randrange(2)
            lead = b"lock " if com == G.COM_AFK and rng.random() < 0.5 else b""
            inpstr = lead + (b"w" * (n - 4) + b" end")[:n]
        else:
            inpstr = rng.choice((b"", b" ")) + rng.choice(WORDS) + rng.choice((b"", b" and more", b"  two  words "))
        wc = 1 + len(sr.words_of(inpstr)) if rng.random() < 0.9 else rng.choice((1, 2))
        events.append((slot, com, inpstr, min(wc, G.MAX_WORDS)))
    return events


def resubmitted(roster: G.Roster, users: dict, rooms, events) -> tuple:
    """The events through the model and the device, the deferred ones again until none is left: the differences, the
    outcomes seen, the calls made."""
    bad, outcomes, calls = [], {}, 0
    while events:
        call = set_call(users, rooms, events)
        got = roster.set_many(events)
        calls += 1
        bad += set_differences(got, call) + mirror_differences(roster, users, rooms)
        for r in call["events"]:
            outcomes[r["outcome"]] = outcomes.get(r["outcome"], 0) + 1
        again = [ev for ev, r in zip(events, call["events"]) if r["outcome"] == G.SET_DEFERRED]
        assert len(again) < len(events)                                 # the first event of a call never defers
        events = again
    return bad, outcomes, calls


def fuzz_part(seed: int, on_device: bool = True) -> dict:
    """Seeded streams over every capacity and every K; without ``on_device`` the model alone, for its outcomes."""
    rng = random.Random(seed)
    bad, outcomes, calls, events_n, colours, actors_seen = [], {}, 0, 0, set(), set()
    for cap in CAPACITIES:
        nr = 3
        rooms, users, actors = fuzz_state(rng, cap, nr)
        colours |= {users[j]["colour"] for j in actors}
        actors_seen |= set(actors)
        if on_device:
            roster = G.Roster(cap, look_rooms=nr)
            set_list_rooms(roster, rooms)
            seat(roster, users)
        for k in EVENTS:
            events = fuzz_events(rng, users, rooms, actors, k)
            events_n += k
            if on_device:
                found, seen, n = resubmitted(roster, users, rooms, events)
                bad += [{"cap": cap, "k": k, **b} for b in found]
                calls += n
            else:
                seen = {}
                while events:
                    call = set_call(users, rooms, events)
                    calls += 1
                    for r in call["events"]:
                        seen[r["outcome"]] = seen.get(r["outcome"], 0) + 1
                    events = [ev for ev, r in zip(events, call["events"]) if r["outcome"] == G.SET_DEFERRED]
            for o, n in seen.items():
                outcomes[o] = outcomes.get(o, 0) + n
        if on_device:
            roster.close()
    return {"capacities": list(CAPACITIES), "events_per_call": list(EVENTS), "calls": calls, "events": events_n,
            "colours": sorted(colours), "edge_slots": sorted(actors_seen & set(EDGE_SLOTS)),
            "outcomes": {str(k): v for k, v in sorted(outcomes.items())}, "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ edges
def edges_state():
    rooms = [list_room(b"den", links=[1]), list_room(b"hall", links=[0])]
    users = {0: set_user(0, name=b"Abcdefghijkl", room=0, colour=1), 63: set_user(63, name=b"Bob", room=0), 64: set_user(64, name=b"Carol", room=0, ignall=1),
             256: set_user(256, name=b"Twelve_bytes", room=1, afk_mesg=b"kept from before"), 5: set_user(5, name=b"Prompt", room=0, login=1),
             6: set_user(6, name=None, room=0)}
    return rooms, users


def edges_part() -> dict:
    """A 12-byte name; an inpstr of ARR_SIZE - 1 bytes for each length-checked command; the actor alone in its room, whose
    here line is planned with nobody admitted; an ``.afk`` that finds a message kept from before."""
    rooms, users = edges_state()
    roster = G.Roster(257, look_rooms=2)
    set_list_rooms(roster, rooms)
    seat(roster, users)
    longest = b"l" * (G.ARR_SIZE - 1)
    bad, out = [], {}
    for label, events in (
            ("twelve", [(0, G.COM_IGNALL, b"", 1), (256, G.COM_TOPIC, b"t" * 60, 2)]),
            ("longest", [(0, com, longest, 2) for com in (G.COM_DESC, G.COM_INPHR, G.COM_OUTPHR, G.COM_TOPIC, G.COM_AFK)]
             + [(63, G.COM_AFK, b"lock " + longest[5:], 3)]),
            ("alone", [(256, G.COM_VIS, b"", 1), (256, G.COM_INVIS, b"", 1)]),
            ("kept", [(256, G.COM_AFK, b"", 1)]), ("kept_lock", [(256, G.COM_AFK, b"lock", 2)])):
        if label.startswith("kept"):
            roster.update(256, vis=1, afk=0)
            users[256].update(vis=1, afk=0)
        found, outcomes, _ = resubmitted(roster, users, rooms, list(events))
        bad += [{"part": label, **b} for b in found]
        out[label] = sorted(outcomes)
    got = roster.set_many([(0, G.COM_IGNALL, b"", 1)])
    out["twelve_here"] = got.here_text(0).decode()
    out["twelve_to"] = np.flatnonzero(got.here.admitted(0)).tolist()
    roster.update(256, afk=0)
    got = roster.set_many([(256, G.COM_AFK, b"", 1)])
    out["kept_here"], out["kept_to"] = got.here_text(0).decode(), np.flatnonzero(got.here.admitted(0)).tolist()
    out["kept_sizes"] = [got.here.variant_sizes[0].tolist(), got.here.write_counts[0].tolist()]
    roster.close()
    return {**out, "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ the calls that follow
def following_part() -> dict:
    """A set_many, then each of the other calls with no update in between: it sees the new state only if the binding
    applied it and the mirrors went up again."""
    rooms = [list_room(b"den", links=[1]), list_room(b"hall", links=[0])]
    users = {0: set_user(0, name=b"Alice", room=0, colour=1, level=3), 1: set_user(1, name=b"Bobby", room=0), 2: set_user(2, name=b"Carol", room=0),
             3: set_user(3, name=b"Dave", room=1)}
    roster = G.Roster(8, look_rooms=2)
    set_list_rooms(roster, rooms)
    seat(roster, users)
    now, date = 1000, b"DATE"
    bad = []

    def settle(events):
        nonlocal bad
        found, _, _ = resubmitted(roster, users, rooms, events)
        bad += [{"after": "set_many", **b} for b in found]

    # speak_many: an ignall listener is not admitted, an invisible speaker is "A presence"
    settle([(2, G.COM_IGNALL, b"", 1), (0, G.COM_INVIS, b"", 1)])
    sp = roster.speak_many([(0, G.COM_SAY, b"hello", 1)])
    if sp.line(0) != b"A presence says: hello\n" or np.flatnonzero(sp.room.admitted(0)).tolist() != [1]:
        bad.append({"after": "speak_many", "line": sp.line(0).decode(), "to": np.flatnonzero(sp.room.admitted(0)).tolist()})
    # tell_many: the AFK message and igntell
    settle([(1, G.COM_AFK, b"gone for tea", 4), (3, G.COM_IGNTELL, b"", 1)])
    for target in (b"bobby", b"dave"):
        want = private(users, 0, G.COM_TELL, target + b" are you there", 4)
        pv = roster.tell_many([(0, G.COM_TELL, target + b" are you there", 4)])
        if pv.reply_text(0) != want["reply"] or pv.line(0) != (want["line"] or b""):
            bad.append({"after": "tell_many", "reply": pv.reply_text(0).decode(), "want": repr(want["reply"])})
    # look_many and who_many: the description, the invisible ARCH, (AFK); rooms_many: the topic
    settle([(1, G.COM_DESC, b"sips ~FGtea", 3), (2, G.COM_TOPIC, b"what is for tea", 5), (0, G.COM_VIS, b"", 1), (3, G.COM_INVIS, b"", 1)])
    for j in (1, 2):
        if roster.look_many([j]).chunks(0) != look_of(users, rooms, j):
            bad.append({"after": "look_many", "slot": j})
        if roster.who_many([j], now=now, date=date).chunks(0) != who_chunks(users, rooms, j, now, date):
            bad.append({"after": "who_many", "slot": j})
        if roster.rooms_many([j], topics=True).chunks(0) != rooms_chunks(users, rooms, j, True):
            bad.append({"after": "rooms_many", "slot": j})
    # go_many: the phrases
    settle([(2, G.COM_INPHR, b"tiptoes in", 3), (2, G.COM_OUTPHR, b"tiptoes", 2)])
    event = [(2, b"hall", 2)]
    call = go_call(users, rooms, [], event, 3, 2)
    bad += [{"after": "go_many", **b} for b in go_differences(roster.go_many(event, gatecrash_level=3, min_private_users=2), call, users, rooms)]
    leave = call["events"][0]["leave"]
    roster.close()
    return {"leave": leave.decode(), "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ repeatability, regrowth
def digest(got: G.Settings) -> str:
    return digest_of(got, [got.reply_colour], texts_of(got))


def determinism_part(seed: int) -> dict:
    runs = []
    for _ in range(2):
        rng = random.Random(seed)
        rooms, users, actors = fuzz_state(rng, 257, 3)
        events = fuzz_events(rng, users, rooms, actors, 64)
        both = []
        for _ in range(2):                                              # the same state twice: a second roster each time
            roster = G.Roster(257, look_rooms=3)
            set_list_rooms(roster, rooms)
            seat(roster, users)
            both.append(digest(roster.set_many(events)))
            roster.close()
        runs.append(both)
    return {"same_on_a_second_call": runs[0][0] == runs[0][1], "same_on_a_second_roster": runs[0] == runs[1]}


def regrown_part(seed: int) -> dict:
    """A small call that changes nothing, then one large enough to make the roster's device allocation grow: the table is
    not dirty, and has to travel again from the pinned mirror."""
    rng = random.Random(seed)
    cap, nr = 65, 3
    rooms, users, actors = fuzz_state(rng, cap, nr)
    roster = G.Roster(cap, look_rooms=nr)
    set_list_rooms(roster, rooms)
    seat(roster, users)
    small = roster.set_many([(actors[0], G.COM_DESC, b"", 1)])
    clean = not (roster._dirty or roster._go_dirty or roster._speech_dirty or roster._set_dirty or roster._afk_dirty or roster._udesc_dirty)
    events = fuzz_events(rng, users, rooms, actors, 600)
    call = set_call(users, rooms, events)
    big = roster.set_many(events)
    bad = set_differences(big, call) + mirror_differences(roster, users, rooms)
    roster.close()
    return {"small_outcome": int(small.outcome[0]), "clean_before": clean, "small_h2d": small.timing["h2d_bytes"],
            "big_h2d": big.timing["h2d_bytes"], "capacity": cap, "events": len(events), "n_bad": len(bad), "first_bad": bad[:2]}


# ------------------------------------------------------------------ the recorded sessions
class SetState(sr.State):
    def login(self, actor: str, name: str) -> None:
        super().login(actor, name)
        u, acc = self.users[self.seats[actor]], self.accounts[name]
        u.update(prompt=int(bool(acc.get("prompt", 0))), charmode_echo=int(bool(acc.get("charmode_echo", 0))), invite=None)

    def everyone(self) -> dict:
        out = super().everyone()
        for u in out.values():
            for f, v in (("prompt", 0), ("charmode_echo", 0), ("in_phrase", b"enters"), ("out_phrase", b"goes"), ("invite", None)):
                u.setdefault(f, v)
        return out


def answer_of(res: dict) -> dict:
    return {"outcome": res["outcome"], "room": res["room"], "reply_colour": res["reply_colour"], "texts": {kind: res[kind] for kind in KINDS},
            "plans": {kind: {"admitted": res["plans"][kind], "chunks": sr.both(res[kind])} for kind in KINDS}}


class SetModelBackend(sr.ModelBackend):
    def set(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        """One event through the model.  It changes ``self.all`` and the state's rooms as the event does."""
        return answer_of(set_call(self.all, self.st.rooms, [(slot, com, inpstr, word_count)])["events"][0])


MORE_FIELDS = ("afk", "afk_mesg", "in_phrase", "out_phrase", "prompt", "charmode_echo")


class SetDeviceBackend(sr.UploadingBackend):
    """One roster for the session.  After a ``set_many`` the replayer's state takes the event's changes and is marked as
    sent: nothing of them is uploaded by ``sync``, so a later call sees what the binding applied."""

    def __init__(self, st):
        super().__init__(st)
        self.more, self.topics = {}, [rm["topic"] for rm in st.rooms]

    def sync(self) -> None:
        super().sync()
        for slot, u in self.st.users.items():
            want = {f: (int(bool(u[f])) if f == "afk" else u[f]) for f in MORE_FIELDS}
            changed = {f: v for f, v in want.items() if self.more.get(slot, {}).get(f, "unset") != v}
            if changed:
                self.roster.update(slot, **changed)
                self.more[slot] = want
        for r, rm in enumerate(self.st.rooms):
            if rm["topic"] != self.topics[r]:
                self.roster.set_rooms(r, topic=rm["topic"])
                self.topics[r] = rm["topic"]

    def set(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        st = self.st
        model = setting(st.users, st.rooms, slot, com, inpstr, word_count)      # for what an effective event changes, no more
        got = self.roster.set_many([(slot, com, inpstr, word_count)])
        self._count("set_many")
        outcome = int(got.outcome[0])
        if outcome in EFFECTIVE and outcome == model["outcome"]:
            apply_set(st.users, st.rooms, model)
            u = st.users[slot]
            self.sent[slot].update({f: u[f] for f in sr.USER_FIELDS})
            self.more[slot] = {f: (int(bool(u[f])) if f == "afk" else u[f]) for f in MORE_FIELDS}
            self.topics = [rm["topic"] for rm in st.rooms]
        return {"outcome": outcome, "room": st.users[slot]["room"], "reply_colour": int(got.reply_colour[0]),
                "texts": {kind: text(0) if got.text_sizes[row, 0] >= 0 else None for row, (kind, _, text) in enumerate(texts_of(got))},
                "plans": {kind: plan_of(plan, 0) for kind, plan, _ in texts_of(got)}}


class SetReplayer(sr.Replayer):
    """The Replayer with the fourteen commands answered: the outcome and the texts come from the backend's ``set``, nothing
    of them from the recording, and the actor's own bytes are compared.  The here lines reach the clones' owners as after
    ``access_many``: composed here from the clone records, as ``relay_many`` relays them -- over the flags as the call
    left them, which is right for every line of these sessions; ``sr.Replayer`` delivers an ``.ignall`` next to a clone of
    the actor's own, from ``Settings.ignall_relays``.  Every other line is ``sr.Replayer``'s, which answers ``.go``,
    ``.clone`` and the rest through the Roster's own event calls; ``UploadingBackend`` then uploads the same state again."""

    def __init__(self, doc: dict, backend_class=SetModelBackend, layout: str = sr.COMPACT):
        self._begin(doc, SetState(doc, layout), backend_class)
        self.res.update(set=0, set_outcomes={}, set_lines=0, returns=0)

    def _compare(self, index: int, step: dict, out: dict, recv: dict) -> None:
        for actor, j in self.st.seats.items():
            got, want = out[j], recv.get(actor, "").encode("latin-1")
            self.res["comparisons"] += 1
            if got != want:
                self.res["mismatches"].append({"step": index, "send": step["send"][:80], "by": step["actor"], "client": actor,
                                               "got": got.decode("latin-1")[:400], "want": want.decode("latin-1")[:400]})

    def _prompt(self, u: dict) -> bytes:
        return nuts_path.transduce(b"~FTCOM> " if u["vis"] else b"~FTCOM+> ", u["colour"]) if u["command_mode"] else b""

    def _here(self, out: dict, text: bytes, rm: int, plan: dict, colour: dict) -> None:
        st = self.st
        for j in plan["admitted"]:
            if j in st.users:
                out[j] += b"".join(plan["chunks"][colour[j]])
        ignall = {j: x["ignall"] for j, x in st.everyone().items()}
        for c in sr.relays(st.records(), ignall, rm, None, text):
            owner = st.clones[c][0]
            out[owner] += b"".join(nuts_path.chunks(sr.relay_text(st.rooms[rm]["name"], text), colour[owner]))

    def _answer(self, index: int, step: dict, u: dict, inp: dict, what: str) -> None:
        st, slot = self.st, u["slot"]
        out = {j: b"" for j in st.users}
        colour = {j: x["colour"] for j, x in st.users.items()}
        a = self.backend.set(slot, inp["com"], inp["inpstr"], inp["word_count"])
        self.res["set"] += 1
        self.res["set_outcomes"][a["outcome"]] = self.res["set_outcomes"].get(a["outcome"], 0) + 1
        if a["outcome"] == G.SET_COLOUR_TEST:                           # the caller's: twenty write_user calls
            out[slot] += b"".join(nuts_path.transduce(line, colour[slot]) for line in G.COLOUR_TEST)
        for kind in ("reply", "reply2"):                                # write_user(user, ...) comes first
            if a["texts"][kind] is not None:
                out[slot] += b"".join(a["plans"][kind]["chunks"][a["reply_colour"]])
        if a["texts"]["here"] is not None:
            self._here(out, a["texts"]["here"], a["room"], a["plans"]["here"], colour)
        if a["outcome"] == G.SET_AFK_LOCKED:                            # the session lock is the caller's
            u["afk"] = 2
        out[slot] += self._prompt(u)
        self.res["commands"][what] = self.res["commands"].get(what, 0) + 1
        self.res["answered"] += 1
        self._compare(index, step, out, step["recv"])

    def _return(self, index: int, step: dict, u: dict):
        """What user_input does for a user who is AFK before anything else (c:180-203), from its format strings.  Returns
        the step with these bytes taken off every client's, or None when the line ends there."""
        st, slot = self.st, u["slot"]
        words = sr.words_of(step["send"].encode("latin-1"))
        out = {j: b"" for j in st.users}
        send = lambda text: out.__setitem__(slot, out[slot] + nuts_path.transduce(text, u["colour"]))
        locked = u["afk"] == 2
        self.res["returns"] += 1
        if locked:
            if not words:
                raise sr.ReplayError(f"step {index}: an empty line to a locked session")
            if words[0] != PASSWORD:
                raise sr.ReplayError(f"step {index}: a wrong password to a locked session")
            for _ in range(5):                                          # cls(), c:2641
                send(b"\n" * 10)
            send(b"Session unlocked, you are no longer AFK.\n")
        else:
            send(b"You are no longer AFK.\n")
        u["afk_mesg"] = b""
        self.backend.sync()
        if u["vis"]:
            self._broadcast(out, [(b"%s comes back from being AFK.\n" % u["name"], u["room"], slot, 0, 0)])
        u["afk"] = 0
        if locked or not words:                                         # c:199-200, 204-211: the line is not run
            out[slot] += self._prompt(u)
            self._compare(index, step, out, step["recv"])
            return None
        recv = {}
        for actor, j in st.seats.items():
            want = step["recv"].get(actor, "").encode("latin-1")
            self.res["comparisons"] += 1
            if not want.startswith(out[j]):
                self.res["mismatches"].append({"step": index, "send": step["send"][:80], "client": actor, "what": "the return from AFK",
                                               "got": out[j].decode("latin-1")[:400], "want": want.decode("latin-1")[:400]})
            recv[actor] = want[len(out[j]):].decode("latin-1")
        return {**step, "recv": recv}

    def line(self, index: int, step: dict) -> None:
        st = self.st
        u = st.users[st.seats[step["actor"]]]
        if (step["send"].split() or [""])[0].lstrip(".") in NAMES:
            self.res["set_lines"] += 1
        if u.get("afk"):
            step = self._return(index, step, u)
            if step is None:
                return
        self.backend.sync()
        inp = self.backend.input(u["slot"], step["send"].encode("latin-1") + b"\n", record=False)
        what = nuts_path.lib().np_command_name(inp["com"]).decode() if inp["kind"] == sr.COMMAND else None
        if what in NAMES:
            self._answer(index, step, u, inp, what)
            return
        super().line(index, step)

    def run(self) -> dict:
        res = super().run()
        res["set_outcomes"] = {str(k): v for k, v in sorted(res["set_outcomes"].items())}
        return res


SESSIONS = ("set",) + tuple(f"replay_{seed}" for seed in sr.FIRST_SEEDS)


def load(name: str) -> dict:
    return load_golden(f"reference_only/{name}.json")


def set_lines(doc: dict) -> int:
    return sum(1 for s in doc["steps"] if s["op"] == "line" and (s["send"].split() or [""])[0].lstrip(".") in NAMES)


def replay_sessions(backend_class=SetModelBackend, layouts=(sr.COMPACT,)) -> dict:
    out = {}
    for name in SESSIONS:
        doc = load(name)
        for layout in layouts if name == "set" else (sr.COMPACT,):
            res = SetReplayer(doc, backend_class, layout).run()
            out[f"{name}:{layout}"] = {"set": res["set"], "set_lines": res["set_lines"], "outcomes": res["set_outcomes"], "returns": res["returns"],
                                      "answered": res["answered"], "tracked": res["tracked"], "comparisons": res["comparisons"],
                                      "mismatches": res["mismatches"][:2], "n_mismatches": len(res["mismatches"]), "capacity": res["capacity"],
                                      "plan_disagreements": res["plan_disagreements"], "calls": res["calls"].get("set_many", 0),
                                      "commands": {k: v for k, v in res["commands"].items() if k in NAMES}}
    return out


def parts(seed: int) -> tuple:
    return (("golden", lambda: replay_sessions(SetDeviceBackend, (sr.COMPACT, sr.SPREAD))), ("fuzz", lambda: fuzz_part(seed)),
            ("edges", edges_part), ("following", following_part), ("determinism", lambda: determinism_part(seed + 1)),
            ("regrown", lambda: regrown_part(seed + 2)))


def profile(res: dict) -> dict:
    golden = res["golden"]
    steps = sum(v["set"] for v in golden.values())
    comparisons = sum(v["comparisons"] for v in golden.values())
    differs = sum(v["n_mismatches"] for v in golden.values()) + sum(res[p]["n_bad"] for p in ("fuzz", "edges", "following", "regrown"))
    return {"steps": steps, "comparisons": comparisons, "verdict": "nothing differs" if not differs else f"{differs} differences",
            "seconds": res["seconds"], "fuzz": {k: res["fuzz"][k] for k in ("calls", "events", "outcomes")},
            "golden": {k: {"set": v["set"], "comparisons": v["comparisons"]} for k, v in golden.items()}}


def main() -> int:
    return child_main("DEVICE_SET", parts, profile, seed=20263)


if __name__ == "__main__":
    sys.exit(main())
