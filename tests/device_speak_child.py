"""The device work of tests/test_device_speak.py, in a short-lived child process of its own, and the CPU model the host
tier of that module shares with it.

As tests/device_review_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_SPEAK {...}``).  ``model`` is the Python model of ``say()``, ``shout()``, ``emote()`` and
``semote()``: the two tables of ``Roster.speak_many`` built from ``np_say_verb`` / ``np_contains_swearing`` of the
restatement and the reference's format strings, each with its nuts333.c line.  ``replay`` runs a recorded session of
tests/golden through an answering function, the model's or the device's.  ``swear_rule`` is the swear scan of
nuts_roster_speak in numpy, with the kernel's slices and overlap.

    python tests/device_speak_child.py [--seed S]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import random
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from device_review_child import Rings  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402

SAY, SHOUT, EMOTE, SEMOTE = device.COM_SAY, device.COM_SHOUT, device.COM_EMOTE, device.COM_SEMOTE
COMS = (SAY, SHOUT, EMOTE, SEMOTE)
MUZZLED_NOTICE = {SAY: b"You are muzzled, you cannot speak.\n",        # nuts333.c:4069
                  SHOUT: b"You are muzzled, you cannot shout.\n",      # nuts333.c:4111
                  EMOTE: b"You are muzzled, you cannot emote.\n",      # nuts333.c:4193
                  SEMOTE: b"You are muzzled, you cannot emote.\n"}     # nuts333.c:4217
WHAT_NOTICE = {SAY: b"Say what?\n",                                    # nuts333.c:4078
               SHOUT: b"Shout what?\n",                                # nuts333.c:4114
               EMOTE: b"Emote what?\n",                                # nuts333.c:4196
               SEMOTE: b"Shout emote what?\n"}                         # nuts333.c:4220
NOSWEARING = b"Swearing is not allowed here.\n"                        # nuts333.h:151, nuts333.c:4092,4117,4199
SWEAR_WORDS = (b"fuck", b"shit", b"cunt")                              # nuts333.h:275-277
GOLDEN = ("swearing", "speech_colour_mixed", "filters", "markup")
#: comparisons each golden session gives: speech steps x logged-in clients
GOLDEN_COMPARISONS = {"swearing": 12, "speech_colour_mixed": 18, "filters": 36, "markup": 20}


# ------------------------------------------------------------------ the model
def model(speaker: dict, com: int, inpstr: bytes, word_count: int, ban_swearing: bool) -> dict:
    """What the command function does for ``speaker`` (slot, room, name, vis, muzzled, command_mode): the outcome, the
    reply to the speaker (None: no write_user call), the room line (None: not spoken) with its (rm, sender), and
    whether it is recorded."""
    lib = nuts_path.lib()
    out = {"outcome": device.SPOKEN, "reply": None, "line": None, "rm": None, "sender": None, "recorded": False}
    byte1 = inpstr[1] if len(inpstr) > 1 else 0                         # past the end: counted as 0
    byte1 = byte1 - 256 if byte1 > 127 else byte1                       # a signed char
    if speaker["muzzled"]:
        return {**out, "outcome": device.MUZZLED, "reply": MUZZLED_NOTICE[com]}
    nothing = {SAY: word_count < 2 and bool(speaker["command_mode"]),   # nuts333.c:4077
               SHOUT: word_count < 2,                                   # nuts333.c:4113
               EMOTE: word_count < 2 and byte1 < 33,                    # nuts333.c:4195
               SEMOTE: word_count < 2 and byte1 < 33}[com]              # nuts333.c:4219
    if nothing:
        return {**out, "outcome": device.NOTHING, "reply": WHAT_NOTICE[com]}
    if ban_swearing and com != SEMOTE and lib.np_contains_swearing(inpstr):       # semote() has no such check
        return {**out, "outcome": device.SWEARING, "reply": NOSWEARING}
    name = speaker["name"] if speaker["vis"] else device.INVISNAME      # nuts333.c:4096 and its like
    slot, room = speaker["slot"], speaker["room"]
    if com == SAY:
        verb = lib.np_say_verb(inpstr)                                  # nuts333.c:4080-4082
        return {**out, "reply": b"You %s: %s\n" % (verb, inpstr),       # nuts333.c:4094
                "line": b"%s %ss: %s\n" % (name, verb, inpstr),         # nuts333.c:4097
                "rm": room, "sender": slot, "recorded": True}           # nuts333.c:4098-4099
    if com == SHOUT:
        return {**out, "reply": b"~OLYou shout:~RS %s\n" % inpstr,      # nuts333.c:4119
                "line": b"~OL%s shouts:~RS %s\n" % (name, inpstr),      # nuts333.c:4122
                "rm": None, "sender": slot}                             # nuts333.c:4123
    if com == EMOTE:
        line = b"%s%s\n" % (name, inpstr[1:]) if inpstr[:1] == b";" else b"%s %s\n" % (name, inpstr)   # c:4202-4203
        return {**out, "line": line, "rm": room, "sender": None, "recorded": True}                     # c:4204-4205
    line = (b"~OL!!~RS %s%s\n" % (name, inpstr[1:]) if inpstr[:1] == b"#"                              # c:4223
            else b"~OL!!~RS %s %s\n" % (name, inpstr))                                                 # c:4224
    return {**out, "line": line, "rm": None, "sender": None}                                           # c:4225


def admitted_by_predicate(roster: device.Roster, rm, sender, com: int) -> np.ndarray:
    """np_fanout_admits over ``roster.table(rm, sender)``, force_listen 0."""
    return np.array([nuts_path.admits(row[:6].tolist(), int(rm is None), 0, com) for row in roster.table(rm, sender)],
                    dtype=bool)


# ------------------------------------------------------------------ the swear scan, as the kernel does it
def swear_rule(texts) -> np.ndarray:
    """nuts_roster_speak's swear scan over a batch of texts (each at most 999 bytes): 64 slices of 16 bytes, each lowered
    (A-Z only) with 3 bytes of overlap and tested for the three words at its 16 positions; any slice's hit is a hit."""
    n = len(texts)
    s = np.zeros((n, 64 * 16 + 3), dtype=np.uint8)
    for r, t in enumerate(texts):
        s[r, :len(t)] = np.frombuffer(t, dtype=np.uint8)
    hit = np.zeros((n, 64), dtype=bool)
    words = [int.from_bytes(w, "little") for w in SWEAR_WORDS]
    for lane in range(64):
        sl = s[:, 16 * lane:16 * lane + 19].astype(np.uint32)
        sl = np.where((sl >= ord("A")) & (sl <= ord("Z")), sl + 32, sl)
        v = sl[:, 0:16] | sl[:, 1:17] << 8 | sl[:, 2:18] << 16 | sl[:, 3:19] << 24
        hit[:, lane] = np.isin(v, words).any(axis=1)
    return hit.any(axis=1)


# ------------------------------------------------------------------ the golden sessions
def wordfind(line: bytes) -> int:
    words = ctypes.create_string_buffer(10 * 41)
    return nuts_path.lib().np_wordfind(line, words)


def classify(send: bytes):
    """A client line as the talker dispatches it: (com, inpstr) of a speech step, a state change's name, or None."""
    first = send.split()[0] if send.split() else b""
    if first in (b".colour", b".ignall", b".ignshout", b".vis", b".invis"):
        return first[1:].decode()
    if first in (b".shout", b"!"):
        return SHOUT, nuts_path.lib().np_remove_first(send)
    if send[:1] in (b".", b">", b"<", b"-"):
        return None
    if send[:1] == b";":
        return EMOTE, send
    if send[:1] == b"#":
        return SEMOTE, send
    return SAY, send


def replay(name: str, answer) -> dict:
    """Session ``name`` of tests/golden: accounts are seated in slots as they log in, all in room 0; the state changes
    are applied; every speech step goes through ``answer(roster, speakers, slot, com, inpstr, word_count, ban)``, which
    returns (reply chunks per colour or None, line chunks per colour or None, admitted bools); every logged-in client's
    bytes are compared with what the reference sent it."""
    doc = json.loads((REPO / "tests" / "golden" / f"{name}.json").read_text())
    ban = bool(doc.get("config", {}).get("ban_swearing", False))
    accounts = {}
    for group in doc["accounts"]:
        for acc in (group if isinstance(group, list) else [group]):
            accounts[acc["name"]] = acc
    roster = device.Roster(8, review_rooms=1)
    seats, speakers = {}, {}
    res = {"comparisons": 0, "speech_steps": 0, "mismatches": [], "outcomes": {}}
    for step in doc["steps"]:
        if step["op"] == "login":
            acc, slot = accounts[step["name"]], len(seats)
            seats[step["actor"]] = slot
            speakers[slot] = {"slot": slot, "room": 0, "name": acc["name"].encode("latin-1"), "vis": 1,
                              "muzzled": int(bool(acc["muzzled"])), "command_mode": int(bool(acc["command_mode"])),
                              "colour": int(bool(acc["colour"])), "ignall": 0, "ignshout": 0}
        elif step["op"] == "line":
            what = classify(step["send"].encode("latin-1"))
            if what is None:
                continue
            sp = speakers[seats[step["actor"]]]
            if isinstance(what, str):
                if what in ("vis", "invis"):
                    sp["vis"] = int(what == "vis")
                else:
                    sp[what] ^= 1
                continue
            for s in speakers.values():
                roster.update(s["slot"], room=s["room"], colour=s["colour"], ignall=s["ignall"], ignshout=s["ignshout"],
                              name=s["name"], vis=s["vis"], muzzled=s["muzzled"], command_mode=s["command_mode"])
            com, inpstr = what
            reply, line, admitted = answer(roster, speakers, sp["slot"], com, inpstr,
                                           wordfind(step["send"].encode("latin-1")), ban)
            res["speech_steps"] += 1
            for actor, slot in seats.items():
                c = speakers[slot]["colour"]
                got = b"".join(reply[c]) if slot == sp["slot"] and reply is not None else b""
                got += b"".join(line[c]) if line is not None and admitted[slot] else b""
                want = step["recv"].get(actor, "").encode("latin-1")
                res["comparisons"] += 1
                if got != want:
                    res["mismatches"].append({"send": step["send"], "actor": actor, "got": got.decode("latin-1"),
                                              "want": want.decode("latin-1")})
    roster.close()
    return res


def model_answer(roster, speakers, slot, com, inpstr, wc, ban):
    m = model(speakers[slot], com, inpstr, wc, ban)
    both = lambda t: None if t is None else {c: nuts_path.chunks(t, c) for c in (0, 1)}
    admitted = (admitted_by_predicate(roster, m["rm"], m["sender"], com) if m["line"] is not None
                else np.zeros(roster.capacity, dtype=bool))
    return both(m["reply"]), both(m["line"]), admitted


# ------------------------------------------------------------------ comparing a Speech with the model
def speech_differences(roster: device.Roster, speakers: dict, events, ban: bool, sp: device.Speech, counts: dict,
                       check_admits: bool = True) -> list:
    """What of a Speech differs from the model: outcome, both texts, both plans' chunks with both colours, who is
    admitted to the room line (np_fanout_admits) and to the reply (the speaker alone)."""
    bad = []
    for k, (slot, com, inpstr, wc) in enumerate(events):
        m = model(speakers[slot], com, inpstr, wc, ban)
        counts[(m["outcome"], com)] = counts.get((m["outcome"], com), 0) + 1
        where = {"event": k, "slot": slot, "com": com, "inpstr": inpstr[:40].decode("latin-1"), "len": len(inpstr),
                 "wc": wc}
        if int(sp.outcome[k]) != m["outcome"]:
            bad.append({**where, "what": "outcome", "device": int(sp.outcome[k]), "model": m["outcome"]})
            continue
        if sp.line(k) != (m["line"] or b"") or sp.reply_text(k) != (m["reply"] or b""):
            bad.append({**where, "what": "text", "device": [sp.line(k)[:60].decode("latin-1"),
                                                             sp.reply_text(k)[:60].decode("latin-1")]})
            continue
        for plan, text, what in ((sp.room, m["line"], "room"), (sp.reply, m["reply"], "reply")):
            for c in (0, 1):
                want = nuts_path.chunks(text, c) if text is not None else []
                if plan.chunks(k, c) != want or int(plan.variant_sizes[k, c]) != sum(map(len, want)):
                    bad.append({**where, "what": f"{what} chunks", "colour": c,
                                "device": [len(x) for x in plan.chunks(k, c)], "model": [len(x) for x in want]})
        want = np.zeros(roster.capacity, dtype=bool)
        if m["reply"] is not None:
            want[slot] = True
        if not np.array_equal(sp.reply.admitted(k), want):
            bad.append({**where, "what": "reply admitted"})
        if m["line"] is None:
            if sp.room.admitted(k).any():
                bad.append({**where, "what": "a line that was not spoken admits someone"})
        elif check_admits:
            want = admitted_by_predicate(roster, m["rm"], m["sender"], com)
            if not np.array_equal(sp.room.admitted(k), want):
                bad.append({**where, "what": "room admitted", "device": int(sp.room.admitted(k).sum()),
                            "model": int(want.sum())})
    return bad


def device_answer(found: dict):
    """replay()'s answering function over speak_many; chunk boundaries are checked against nuts_path.chunks of the
    model's texts on the way (``found``)."""
    def answer(roster, speakers, slot, com, inpstr, wc, ban):
        sp = roster.speak_many([(slot, com, inpstr, wc)], ban_swearing=ban)
        bad = speech_differences(roster, speakers, [(slot, com, inpstr, wc)], ban, sp, found.setdefault("counts", {}))
        found.setdefault("bad", []).extend(bad)
        both = lambda plan, there: {c: plan.chunks(0, c) for c in (0, 1)} if there else None
        return both(sp.reply, bool(sp.reply_text(0))), both(sp.room, bool(sp.line(0))), sp.room.admitted(0)
    return answer


# ------------------------------------------------------------------ seeded events
def fuzz_inpstr(rng: random.Random) -> bytes:
    rb = lambda n: bytes(rng.randrange(1, 256) for _ in range(n))
    words = lambda n: b" ".join(rng.choice((b"hello", b"there", b"a", b"Scunthorpe", b"x" * 17, b"~FRred", b"/~OL", b"~RS",
                                            b"?", b"wh\xe9re")) for _ in range(n))
    x = rng.random()
    if x < 0.15:
        t = rb(rng.choice((0, 1, 2, 3, 15, 16, 17, rng.randrange(1000), rng.randrange(1000), 999)))
    elif x < 0.35:                                                      # a planted swear word, any case, anywhere
        w = bytes(rng.choice((ch, ch ^ 32)) for ch in rng.choice(SWEAR_WORDS))
        if rng.random() < 0.25:                                         # ... or a near miss
            w = rng.choice((w[:3], w[:2] + b" " + w[2:], w[1:], w[:3] + b"\xeb", b"fuc\n", w[:3] + bytes([w[3] ^ 0x80])))
        room = 999 - len(w)
        before = rng.choice((0, 0, room, rng.randrange(room + 1), 16 * rng.randrange(1, 60) - rng.randrange(0, 5)))
        before = min(before, room)
        after = rng.choice((0, 0, room - before, rng.randrange(room - before + 1)))
        t = (words(200) + b" " * 999)[:before] + w + words(200)[:after]
    elif x < 0.5:
        t = words(rng.randrange(1, 30))[:998] + rng.choice((b"?", b"!", b"?!", b"!?", b"? ", b"."))
    elif x < 0.62:
        t = rng.choice((b";", b"#", b"; ", b"# ", b";\n", b"#\x80")) + words(rng.randrange(0, 12))
    elif x < 0.72:
        t = b"".join(rng.choice((b"~FR", b"~RS", b"~OL", b"/~", b"~", b"/", b"~B", b"ab", b" ")) for _ in range(rng.randrange(1, 300)))
    elif x < 0.82:
        t = b"".join(rng.choice((b"\n", b"\n", b"\n", b"x", b"~FG")) for _ in range(rng.randrange(1, 999)))
    elif x < 0.9:
        t = rng.choice((b"\n" * 999, b"x" * 999, b"~FR" * 333, b"x" * 995 + b"shit", b"FUCK" + b"\n" * 995, b"\n" * 998 + b"?",
                        b";" + b"\n" * 998, b"#" + b"~RS" * 332 + b"!", b"x" * 994 + b"cunt" + b"!"))
    else:
        t = rng.choice((b"", b";", b"#", b"a", b"?", b"!", b"; x", b"#x", b";x", b"# ", b"a?", b"hi", b";\xe9", b"shit", b"cun"))
    return t[:999].replace(b"\0", b"\x01")


def random_roster(rng: random.Random, cap: int, review_rooms: int = 0):
    """A roster of ``cap`` slots in a random state, the speakers' side of it as model() takes it, and the valid
    speakers: a room, no login flag, a name."""
    roster = device.Roster(cap, review_rooms=review_rooms)
    speakers, valid = {}, []
    rooms = [None, 0, 0, 1, 2]
    for j in range(cap):
        if rng.random() < 0.7:
            name = bytes(rng.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz") for _ in range(rng.randrange(1, 13)))
        elif rng.random() < 0.5:
            name = bytes(rng.randrange(1, 256) for _ in range(rng.choice((1, 12, rng.randrange(1, 13)))))
        else:
            name = None
        s = {"slot": j, "room": rng.choice(rooms), "name": name, "vis": int(rng.random() < 0.7),
             "muzzled": int(rng.random() < 0.15), "command_mode": int(rng.random() < 0.4)}
        flags = {"login": int(rng.random() < 0.1), "ignall": int(rng.random() < 0.2),
                 "ignshout": int(rng.random() < 0.3), "colour": rng.randrange(2)}
        if j == 0:                                                      # one speaker at least
            s.update(room=0, name=s["name"] or b"Zero")
            flags["login"] = 0
        roster.update(j, room=s["room"], vis=s["vis"], muzzled=s["muzzled"], command_mode=s["command_mode"], **flags)
        if s["name"] is not None:
            roster.update(j, name=s["name"])
        speakers[j] = s
        if s["room"] is not None and not flags["login"] and s["name"] is not None:
            valid.append(j)
    return roster, speakers, valid


CAPACITIES = (1, 63, 64, 65, 300, 1000)
EVENTS_PER_CALL = 300


def fuzz_part(seed: int) -> dict:
    rng = random.Random(seed)
    counts: dict = {}
    res = {"capacities": [], "calls": 0, "events": 0, "n_bad": 0, "first_bad": [], "longest_inpstr": 0,
           "copies": []}
    for cap in CAPACITIES:
        roster, speakers, valid = random_roster(rng, cap)
        with roster:
            res["capacities"].append(cap)
            for ban in (False, True):
                events = [(rng.choice(valid), rng.choice(COMS), fuzz_inpstr(rng), rng.randrange(11))
                          for _ in range(EVENTS_PER_CALL)]
                sp = roster.speak_many(events, ban_swearing=ban)
                bad = speech_differences(roster, speakers, events, ban, sp, counts)
                # both plans expand: the reply plan gives each speaker its own text, nobody else anything
                for plan in (sp.room, sp.reply):
                    f = plan.expand()
                    if int(f.admitted.sum()) != sum(int(plan.admitted(k).sum()) for k in range(len(events))):
                        bad.append({"what": "expand admits another count"})
                res["n_bad"] += len(bad)
                res["first_bad"] += bad[:5 - len(res["first_bad"])]
                res["calls"] += 1
                res["events"] += len(events)
                res["longest_inpstr"] = max(res["longest_inpstr"], max(len(e[2]) for e in events))
                res["copies"].append([cap, len(events), sp.timing["h2d_bytes"], sp.timing["d2h_bytes"]])
    res["outcome_by_com"] = {f"{o}/{c}": n for (o, c), n in sorted(counts.items())}
    return res


def contract_part(seed: int) -> dict:
    """sp.room at k equals plan_many([(sp.line(k), rm_k, sender_k, 0, com_k)]) at 0, field by field."""
    rng = random.Random(seed)
    res = {"checked": 0, "n_bad": 0, "first_bad": [], "coms": set()}
    for cap in (65, 300):
        roster, speakers, valid = random_roster(rng, cap)
        with roster:
            events = [(rng.choice(valid), rng.choice(COMS), fuzz_inpstr(rng), rng.randrange(11)) for _ in range(120)]
            sp = roster.speak_many(events)
            spoken = [k for k in range(len(events)) if sp.outcome[k] == device.SPOKEN]
            for k in spoken[:40]:
                slot, com, inpstr, wc = events[k]
                m = model(speakers[slot], com, inpstr, wc, False)
                p = roster.plan_many([(sp.line(k), m["rm"], m["sender"], 0, com)])
                same = (np.array_equal(sp.room.admitted_bits[k], p.admitted_bits[0])
                        and np.array_equal(sp.room.colour_bits, p.colour_bits) and sp.room.capacity == p.capacity
                        and np.array_equal(sp.room.variant_sizes[k], p.variant_sizes[0])
                        and np.array_equal(sp.room.write_counts[k], p.write_counts[0])
                        and all(sp.room.variant(k, c) == p.variant(0, c) and sp.room.chunks(k, c) == p.chunks(0, c)
                                and np.array_equal(sp.room.recipients(k, c), p.recipients(0, c)) for c in (0, 1)))
                res["checked"] += 1
                res["coms"].add(com)
                if not same:
                    res["n_bad"] += 1
                    res["first_bad"] += [{"event": k, "com": com, "len": len(inpstr)}][:5 - len(res["first_bad"])]
    res["coms"] = sorted(res["coms"])
    return res


def recording_part(seed: int) -> dict:
    """speak_many(record=True), plan_many(record=), clear_review and review_many interleaved, against Rings."""
    rng = random.Random(seed)
    rr, cap = 3, 40
    res = {"speak_calls": 0, "plan_calls": 0, "clears": 0, "reviews": 0, "lines_compared": 0, "n_bad": 0,
           "first_bad": [], "recorded": 0, "not_recorded": {"shout": 0, "semote": 0, "unspoken": 0},
           "most_into_one_room_in_one_call": 0}
    roster, speakers, valid = random_roster(rng, cap, review_rooms=rr)
    rings = Rings(rr)

    def review():
        rooms = list(range(rr))
        rv = roster.review_many(rooms)
        for q in rooms:
            want = rings.lines(q)
            res["lines_compared"] += len(want)
            if rv.lines(q) != want or any(rv.chunks(q, c) != rings.chunks(q, c) for c in (0, 1)):
                res["n_bad"] += 1
                res["first_bad"] += [{"room": q, "device": len(rv.lines(q)), "model": len(want)}][:5 - len(res["first_bad"])]
        res["reviews"] += 1

    with roster:
        steps = ["speak", "speak", "plan", "clear", "review", "speak_plain"] * 5 + ["speak"] * 4
        rng.shuffle(steps)
        for op in steps + ["review"]:
            if op == "review":
                review()
            elif op == "clear":
                rooms = [rng.randrange(rr) for _ in range(rng.randint(1, 2))]
                roster.clear_review(rooms)
                for rm in rooms:
                    rings.clear(rm)
                res["clears"] += 1
            elif op == "plan":
                calls = [(fuzz_inpstr(rng), rng.randrange(rr), None, 0, SAY) for _ in range(rng.choice((1, 5, 40)))]
                roster.plan_many(calls, record=True)
                for t, rm, *_ in calls:
                    rings.record(rm, t)
                res["plan_calls"] += 1
            else:
                k = rng.choice((1, 7, 64, 200))
                ban = rng.random() < 0.5
                events = [(rng.choice(valid), rng.choice(COMS), fuzz_inpstr(rng), rng.randrange(11)) for _ in range(k)]
                sp = roster.speak_many(events, ban_swearing=ban, record=op == "speak")
                per_room: dict = {}
                for j, (slot, com, inpstr, wc) in enumerate(events):
                    m = model(speakers[slot], com, inpstr, wc, ban)
                    if int(sp.outcome[j]) != m["outcome"] or sp.line(j) != (m["line"] or b""):
                        res["n_bad"] += 1
                    if op != "speak":
                        continue
                    if m["recorded"]:
                        rings.record(m["rm"], m["line"])
                        per_room[m["rm"]] = per_room.get(m["rm"], 0) + 1
                        res["recorded"] += 1
                    else:
                        res["not_recorded"]["unspoken" if m["line"] is None else
                                            "shout" if com == SHOUT else "semote"] += 1
                res["most_into_one_room_in_one_call"] = max([res["most_into_one_room_in_one_call"], *per_room.values()])
                res["speak_calls"] += 1
                if rng.random() < 0.5:
                    review()
    return res


def nothing_else_moved_part() -> dict:
    """plan_many and broadcast_many give the same results and upload the same bytes before and after speak_many calls
    and after an update of the speech fields alone."""
    out = {}
    rng = random.Random(7)
    roster, speakers, valid = random_roster(rng, 300)
    calls = [(b"Uaaa says: line %d ~FRred~RS\n" % i, rng.choice((None, 0, 1)), rng.choice((None, 5)), 0, SAY)
             for i in range(20)]
    events = [(rng.choice(valid), rng.choice(COMS), fuzz_inpstr(rng), rng.randrange(11)) for _ in range(100)]

    def snapshot():
        p, f = roster.plan_many(calls), roster.broadcast_many(calls)
        return {"plan": [p.admitted_bits.tobytes().hex()[:64], [p.variant(k, c).hex() for k in range(3) for c in (0, 1)],
                         p.variant_sizes.tolist(), p.write_counts.tolist(), int(p.admitted_bits.view(np.uint8).sum())],
                "fanout": [int(f.admitted.sum()), int(f.out_offsets[-1]), int(f.write_offsets[-1]),
                           f.arena[:2000].tobytes().hex()],
                "plan_copies": [p.timing["h2d_bytes"], p.timing["d2h_bytes"]],
                "fanout_copies": [f.timing["h2d_bytes"], f.timing["d2h_bytes"]]}

    with roster:
        snapshot()                                   # every kind of call once: the allocations have their sizes
        first = roster.speak_many(events).timing
        snapshot()
        out["before"] = snapshot()
        a = roster.speak_many(events).timing
        b = roster.speak_many(events, ban_swearing=True).timing
        out["after_speaking"] = snapshot()
        dirty_before = roster._dirty
        roster.update(valid[0], name=b"Renamed", muzzled=1, vis=0, command_mode=1)
        out["speech_update_left_dirty"] = [dirty_before, roster._dirty]
        out["after_speech_update"] = snapshot()
        c = roster.speak_many(events).timing
        d = roster.speak_many(events).timing
        out["after_speaking_again"] = snapshot()
        roster.update(valid[0], colour=1)
        e = roster.speak_many(events).timing
        out["speak_h2d"] = {"first": first["h2d_bytes"], "clean": [a["h2d_bytes"], b["h2d_bytes"], d["h2d_bytes"]],
                            "after_speech_update": c["h2d_bytes"], "after_table_update": e["h2d_bytes"]}
        out["speak_d2h"] = sorted({t["d2h_bytes"] for t in (first, a, b, c, d, e)})
        out["capacity"] = roster.capacity
    return out


def golden_part() -> dict:
    out = {}
    for name in GOLDEN:
        found: dict = {}
        res = replay(name, device_answer(found))
        res["n_bad_vs_model"] = len(found.get("bad", []))
        res["first_bad_vs_model"] = found.get("bad", [])[:3]
        res["mismatches"] = res["mismatches"][:3]
        out[name] = res
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1701)
    a = ap.parse_args()
    out = {"device_count": device.device_count()}
    if out["device_count"] < 1:
        print("device_speak_child: no GPU visible", file=sys.stderr)
        return 2
    out["golden"] = golden_part()
    out["fuzz"] = fuzz_part(a.seed)
    out["contract"] = contract_part(a.seed + 1)
    out["recording"] = recording_part(a.seed + 2)
    out["moved"] = nothing_else_moved_part()
    print("DEVICE_SPEAK " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
