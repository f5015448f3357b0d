"""The device work of tests/test_device_relay.py, in a short-lived child process of its own, and the CPU model the host
tier of that module shares with it.

As tests/device_look_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_RELAY {...}``).  ``relays`` and ``relay_text`` are the Python model of the clone branch of
``write_room_except`` (nuts333.c:1416-1426); the variants of a relay text come from ``nuts_path.chunks``.  ``replay_relays``
runs the recorded ``clones`` session of tests/golden: it tracks the users' rooms, their ``ignall`` and the clones from the
commands the session sends, and compares what the model relays in every ``line`` step with the recorded relay lines.

    python tests/device_relay_child.py [--seed S]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import random
import re
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from device_look_child import copies, default_rooms, other_calls, plan_digest  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402

NOTHING, SWEARS, ALL = device.CLONE_HEAR_NOTHING, device.CLONE_HEAR_SWEARS, device.CLONE_HEAR_ALL
CAPACITIES = (1, 64, 65, 257)
CLONES = (1, 63, 64, 65, 257)
BROADCASTS_PER_CALL = 32
#: room names at the edges: 1 and 20 bytes, colour markup and a slash in a name
ROOM_NAMES = (b"d", b"N" * 20, b"hallway", b"~FRred/", b"wiz")
RELAY_LINE = re.compile(r"^\[ (\S+) \]: ")


# ------------------------------------------------------------------ the model
def swearing(text: bytes) -> bool:
    return bool(nuts_path.lib().np_contains_swearing(text))


def relays(records, ignall, rm, clone_sender, text: bytes) -> list:
    """The clone records that relay a broadcast of ``text`` to room ``rm`` (None: every room), ascending.  ``records`` is a
    sequence of ``(owner, room, hear)`` with owner None for an empty record, ``ignall`` maps a slot to its flag, and
    ``clone_sender`` is the record that is ``user`` of the broadcast, or None."""
    if rm is None:
        return []
    out = []
    for c, (owner, room, hear) in enumerate(records):
        if owner is None or room != rm or c == clone_sender or hear == NOTHING or ignall[owner]:
            continue
        if hear == ALL or swearing(text):
            out.append(c)
    return out


def relays_of(records, ignall, broadcast, clone_sender=None) -> list:
    """``relays`` for a whole ``(text, rm, sender, force_listen, com_num)`` tuple: the rule reads its text and its room."""
    text, rm, _sender, _force_listen, _com_num = broadcast
    return relays(records, ignall, rm, clone_sender, text)


def relay_text(name: bytes, text: bytes) -> bytes:
    return b"~FT[ " + name + b" ]:~RS " + text


def longest_text(name: bytes) -> int:
    """The longest broadcast a room of that name with a clone in it takes: the relay text fills text2[ARR_SIZE]."""
    return device.ARR_SIZE - 1 - device.RELAY_EXTRA - len(name)


# ------------------------------------------------------------------ the recorded session
def recorded_relays(doc) -> dict:
    """{step index: {actor: [line, ...]}} of the recv lines that begin ``[ <room> ]: ``."""
    out = {}
    for i, step in enumerate(doc["steps"]):
        for who, text in step.get("recv", {}).items():
            lines = [l for l in text.split("\n\r") if RELAY_LINE.match(l)]
            if lines:
                out.setdefault(i, {})[who] = lines
    return out


def replay_relays(name: str = "clones") -> dict:
    """Session ``name`` of tests/golden through the model.  Users are seated in login order in room 0; the clones are kept in
    the order they were created, as the talker's user list keeps them.  Every command the session sends is either applied
    -- the broadcasts it makes are listed as ``(rm, text, clone_sender)`` from the reference's format strings -- or known
    to make no room broadcast; an unknown command is an error.  For every ``line`` step the model's relay lines per actor,
    transduced without colour, are compared with the recorded ones."""
    doc = json.loads((REPO / "tests" / "golden" / f"{name}.json").read_text())
    accounts = {}
    for group in doc["accounts"]:
        for acc in (group if isinstance(group, list) else [group]):
            accounts[acc["name"]] = acc
    rooms = [r["name"] for r in default_rooms()]
    max_clones = int(doc["config"].get("max_clones", 1))
    users, order, clones = {}, [], []                      # actor -> user; slots in login order; [owner actor, room, hear]
    recorded = recorded_relays(doc)
    res = {"line_steps": 0, "relay_lines": 0, "relay_entries": 0, "compared_steps": [], "mismatches": [], "commands": {}}

    def room_named(word: bytes):
        return next((i for i, n in enumerate(rooms) if n.startswith(word)), None)       # get_room, c:2412

    def find_clone(owner, rm):
        return next((i for i, c in enumerate(clones) if c[0] == owner and c[1] == rm), None)

    def broadcasts_of(actor: str, line: bytes) -> list:
        u = users[actor]
        me = u["name"]
        if line.startswith(b";"):                                        # emote(), c:4202-4204
            res["commands"]["emote"] = res["commands"].get("emote", 0) + 1
            return [(u["room"], me + line[1:] + b"\n", None)]
        if not line.startswith(b"."):                                    # say(), c:4080-4098
            res["commands"]["say"] = res["commands"].get("say", 0) + 1
            verb = {b"?": b"ask", b"!": b"exclaim"}.get(line[-1:], b"say")
            return [(u["room"], b"%s %ss: %s\n" % (me, verb, line), None)]
        words = line.split()
        com = words[0][1:].decode()
        res["commands"][com] = res["commands"].get(com, 0) + 1
        if com in ("look", "myclones", "review", "tell"):                # they write to users, not to rooms
            return []
        if com == "shout":                                               # to every room: never relayed
            return [(None, b"~OL%s shouts:~RS %s\n" % (me, line.split(None, 1)[1]), None)]
        if com == "go":                                                  # move_user, c:4451-4453
            rm = room_named(words[1])
            old, u["room"] = u["room"], rm
            return [(rm, b"%s %s.\n" % (me, u["in_phrase"]), None),
                    (old, b"%s %s to the %s.\n" % (me, u["out_phrase"], rooms[rm]), None)]
        if com == "clone":                                               # create_clone, c:7100-7160
            rm = room_named(words[1]) if len(words) > 1 else u["room"]
            mine = [c for c in clones if c[0] == actor]
            if any(c[1] == rm for c in mine) or len(mine) >= max_clones:
                return []
            clones.append([actor, rm, ALL])
            return [(u["room"], b"~FB~OL%s whispers a haunting spell...\n" % me, None),
                    (rm, b"~FB~OLA clone of %s appears in a swirling magical mist!\n" % me, None)]
        if com == "destroy":                                             # destroy_clone, c:7165-7209
            rm = room_named(words[1]) if len(words) > 1 else u["room"]
            whose = actor
            if len(words) > 2:
                whose = next(a for a, v in users.items() if v["name"].lower().startswith(words[2].lower()))
                if users[whose]["level"] >= u["level"]:
                    return []
            i = find_clone(whose, rm)
            if i is None:
                return []
            del clones[i]
            return [(u["room"], b"~FM~OL%s whispers a sharp spell...\n" % me, None),
                    (rm, b"~FM~OLThe clone of %s shimmers and vanishes.\n" % users[whose]["name"], None)]
        if com == "switch":                                              # clone_switch, c:7263-7289
            i = find_clone(actor, room_named(words[1])) if len(words) > 1 else None
            if i is None:
                return []
            clones[i][1], u["room"] = u["room"], clones[i][1]
            return [(u["room"], b"The clone of %s comes alive!\n" % me, None),
                    (clones[i][1], b"%s turns into a clone!\n" % me, i)]         # write_room_except(u->room, text, u)
        if com == "chear":                                               # clone_hear, c:7320-7357
            mode = {b"all": ALL, b"swears": SWEARS, b"nothing": NOTHING}.get(words[2] if len(words) > 2 else b"")
            i = find_clone(actor, room_named(words[1])) if mode is not None else None
            if i is not None:
                clones[i][2] = mode
            return []
        if com == "csay":                                                # clone_say -> say(clone), c:4085-4088
            i = find_clone(actor, room_named(words[1])) if len(words) > 2 else None
            if i is None:
                return []
            said = line.split(None, 2)[2]
            verb = {b"?": b"ask", b"!": b"exclaim"}.get(said[-1:], b"say")
            return [(clones[i][1], b"Clone of %s %ss: %s\n" % (me, verb, said), None)]   # write_room: nobody is left out
        if com == "ignall":                                              # toggle_ignall, c:4463-4477: the flag flips last
            text = b"%s is now ignoring everyone.\n" % me if not u["ignall"] else b"%s is listening again.\n" % me
            return [(u["room"], text, None, ("ignall", actor))]
        raise AssertionError(f"the session sends a command the replay does not know: {line!r}")

    for i, step in enumerate(doc["steps"]):
        if step["op"] == "login":
            acc = accounts[step["name"]]
            users[step["actor"]] = {"name": acc["name"].encode("latin-1"), "room": 0, "ignall": 0, "level": int(acc["level"]),
                                    "in_phrase": acc["in_phrase"].encode("latin-1"),
                                    "out_phrase": acc["out_phrase"].encode("latin-1"), "slot": len(order)}
            order.append(step["actor"])
        elif step["op"] == "close" and step.get("actor") in users:       # the owner leaves, its clones with it
            clones[:] = [c for c in clones if c[0] != step["actor"]]
            users[step["actor"]]["room"] = None
        elif step["op"] == "line":
            res["line_steps"] += 1
            got = {}
            for bc in broadcasts_of(step["actor"], step["send"].encode("latin-1")):
                rm, text, csender = bc[:3]
                records = [(users[c[0]]["slot"], c[1], c[2]) for c in clones]
                ignall = {u["slot"]: u["ignall"] for u in users.values()}
                for c in relays(records, ignall, rm, csender, text):
                    line = nuts_path.transduce(relay_text(rooms[rm], text), 0).decode("latin-1")
                    assert line.endswith("\n\r")
                    got.setdefault(clones[c][0], []).append(line[:-2])
                if len(bc) > 3:
                    users[bc[3][1]]["ignall"] ^= 1
            want = recorded.get(i, {})
            res["relay_lines"] += sum(len(v) for v in got.values())
            res["relay_entries"] += len(got)
            if want:
                res["compared_steps"].append(i)
            if got != want:
                res["mismatches"].append({"step": i, "send": step["send"], "model": got, "recorded": want})
            for who, lines in want.items():                              # a direct listener of the step got the same bytes
                for l in lines:
                    after = l[RELAY_LINE.match(l).end():]
                    direct = [w for w, text in step["recv"].items() if w != who and after + "\n\r" in text]
                    rm_name = RELAY_LINE.match(l).group(1)
                    if not direct and any(users[a]["room"] is not None and rooms[users[a]["room"]].decode() == rm_name
                                          and a != step["actor"] and a != who for a in users):
                        res["mismatches"].append({"step": i, "what": "no direct listener shows the relayed line", "line": l})
    res["recorded_lines"] = sum(len(l) for v in recorded.values() for l in v.values())
    res["recorded_entries"] = sum(len(v) for v in recorded.values())
    return res


# ------------------------------------------------------------------ seeded rosters
def fuzz_roster(rng: random.Random, cap: int, nclones: int, **kw):
    """A roster of ``cap`` slots and ``nclones`` clone records over five named rooms; room 4 never holds a clone."""
    roster = device.Roster(cap, look_rooms=len(ROOM_NAMES), clones=nclones, **kw)
    roster.set_rooms(list(range(len(ROOM_NAMES))), name=list(ROOM_NAMES))
    users = {j: {"room": rng.choice((0, 1, 2, 3, 4, None)), "ignall": int(rng.random() < 0.25), "colour": rng.randrange(2),
                 "login": int(rng.random() < 0.1), "ignshout": rng.randrange(2)} for j in range(cap)}
    roster.update(list(range(cap)), **{f: [users[j][f] for j in range(cap)] for f in ("room", "ignall", "colour", "login", "ignshout")})
    records = []
    for c in range(nclones):
        empty = rng.random() < 0.15
        records.append([None if empty else rng.randrange(cap), rng.randrange(4), rng.choice((NOTHING, SWEARS, ALL))])
    for c in sorted({0, 62, 63, 64, 255, 256, nclones - 1} & set(range(nclones))):       # the bitmap's edges relay
        records[c] = [rng.randrange(cap), 0, ALL]
    put_records(roster, records)
    return roster, users, records


def put_records(roster, records, which=None) -> None:
    for c in (range(len(records)) if which is None else which):
        owner, room, hear = records[c]
        if owner is None:
            roster.set_clones(c, owner=None)
        else:
            roster.set_clones(c, owner=owner, room=room, hear=hear)


TEXTS = (b"", b"hello\n", b"Alice says: ~FRred~RS and /~FG escaped\n", b"a SHIT line\n", b"what the FuCk", b"cunt", b"\n" * 40,
         b"~FR" * 50, b"/~" * 60, b"ends in a slash/", b"\xe9\xff high \x80 bytes\n", b"x" * 400 + b"\n")


def fuzz_broadcasts(rng: random.Random, cap: int, records, counts) -> tuple:
    cloned = {r[1] for r in records if r[0] is not None}
    bs, csenders = [], []
    for k in range(BROADCASTS_PER_CALL):
        rm = rng.choice((0, 0, 0, 1, 2, 3, 4, 77, None))
        text = rng.choice(TEXTS)
        if rm in cloned and rng.random() < 0.2:                        # exactly the longest text the room takes
            text = (b"shit " if rng.random() < 0.5 else b"") + b"L" * device.ARR_SIZE
            text = text[:longest_text(ROOM_NAMES[rm]) - 1] + b"\n"
            counts["at_limit"] += 1
        csender = None
        if rm is not None and rm < 4 and rng.random() < 0.3:
            here = [c for c, r in enumerate(records) if r[0] is not None and r[1] == rm]
            csender = rng.choice(here) if here else rng.randrange(len(records))
        sender = None if csender is not None or rng.random() < 0.3 else rng.randrange(cap)
        bs.append((text, rm, sender, rng.randrange(2), rng.choice((0, 3, 4, 7))))
        csenders.append(csender)
    return bs, csenders


def relay_differences(roster, users, records, bs, csenders, rl: device.Relay, counts, names=ROOM_NAMES) -> list:
    """``names`` maps a room to its name: the fuzz rosters' ROOM_NAMES, or a dict for a roster with other rooms."""
    bad = []
    ignall = {j: u["ignall"] for j, u in users.items()}
    for k, ((text, rm, sender, fl, com), cs) in enumerate(zip(bs, csenders)):
        want = relays(records, ignall, rm, cs, text)
        here = [r for r in records if r[0] is not None and r[1] == rm]
        counts["rm_none"] += rm is None
        counts["no_clone_room"] += rm is not None and not here
        counts["empty_text"] += text == b""
        counts["clone_sender"] += cs is not None
        counts["clone_sender_excluded"] += cs is not None and records[cs][0] is not None and records[cs][1] == rm
        counts["hear"] |= {r[2] for r in here}
        counts["ignall_owner"] += sum(1 for r in here if ignall[r[0]] and r[2] != NOTHING)
        counts["forced_past_ignall"] += sum(1 for r in here if ignall[r[0]] and fl)
        counts["swear_relays"] += sum(1 for c in want if records[c][2] == SWEARS)
        counts["relays"] += len(want)
        counts["most_relays"] = max(counts["most_relays"], len(want))
        counts["most_words"] = max(counts["most_words"], len({c // 64 for c in want}))
        counts["edge_relays"] += sum(1 for c in want if c in (63, 64, 256))
        where = {"broadcast": k, "rm": rm, "clone_sender": cs, "text": text[:40].decode("latin-1")}
        flags = np.zeros(len(records), dtype=bool)
        flags[want] = True
        if rl.relay_bits[k].tolist() != device._pack(flags).tolist():      # whole words: the tail bits are zero
            bad.append({**where, "what": "bitmap", "device": rl.relays(k).tolist()[:20], "model": want[:20]})
            continue
        if rl.owners(k).tolist() != [records[c][0] for c in want]:
            bad.append({**where, "what": "owners"})
        counts["owner_colours"] |= {int(users[records[c][0]]["colour"]) for c in want}
        if rl.owner_colours(k).tolist() != [users[records[c][0]]["colour"] for c in want]:
            bad.append({**where, "what": "owner colours"})
        model = relay_text(names[rm], text) if want else b""
        if rl.relay_text(k) != model:
            bad.append({**where, "what": "text", "device": rl.relay_text(k)[:60].decode("latin-1")})
        for c in (0, 1):
            ch = nuts_path.chunks(model, c) if want else []
            if rl.relay_chunks(k, c) != ch or rl.relay_variant(k, c) != b"".join(ch):
                bad.append({**where, "what": "variant", "colour": c, "device": [len(x) for x in rl.relay_chunks(k, c)],
                            "model": [len(x) for x in ch]})
    return bad


def new_counts() -> dict:
    return {"rm_none": 0, "no_clone_room": 0, "empty_text": 0, "clone_sender": 0, "clone_sender_excluded": 0, "hear": set(),
            "ignall_owner": 0, "forced_past_ignall": 0, "swear_relays": 0, "relays": 0, "most_relays": 0, "most_words": 0, "edge_relays": 0, "at_limit": 0,
            "owner_colours": set()}


# ------------------------------------------------------------------ the parts of the device run
def fuzz_part(seed: int) -> dict:
    rng = random.Random(seed)
    counts, bad, calls = new_counts(), [], 0
    for cap in CAPACITIES:
        for nclones in CLONES:
            roster, users, records = fuzz_roster(rng, cap, nclones)
            for _ in range(2):
                bs, csenders = fuzz_broadcasts(rng, cap, records, counts)
                rl = roster.relay_many(bs, clone_sender=csenders)
                bad += relay_differences(roster, users, records, bs, csenders, rl, counts)
                calls += 1
                c, j = rng.randrange(nclones), rng.randrange(cap)           # something changes between the calls
                records[c] = [rng.randrange(cap), rng.randrange(4), rng.choice((SWEARS, ALL))]
                put_records(roster, records, [c])
                users[j]["ignall"] ^= 1
                roster.update(j, ignall=users[j]["ignall"])
            roster.close()
    out = {k: (sorted(v) if isinstance(v, set) else int(v)) for k, v in counts.items()}
    return {"capacities": list(CAPACITIES), "clones": list(CLONES), "calls": calls, "broadcasts": calls * BROADCASTS_PER_CALL,
            **out, "n_bad": len(bad), "first_bad": bad[:1]}


def plan_differences(a: device.Plan, b: device.Plan) -> list:
    bad = []
    for f in ("admitted_bits", "colour_bits", "variant_starts", "variant_sizes", "write_counts"):
        if not np.array_equal(getattr(a, f), getattr(b, f)):
            bad.append(f)
    if a.capacity != b.capacity or sorted(a.timing) != sorted(b.timing):
        bad.append("capacity or timing keys")
    for k in range(len(a.admitted_bits)):
        for c in (0, 1):
            if a.variant(k, c) != b.variant(k, c) or a.chunks(k, c) != b.chunks(k, c):
                bad.append(f"variant ({k}, {c})")
    return bad


def contract_part(seed: int) -> dict:
    rng = random.Random(seed)
    counts = new_counts()
    rosters = []
    for _ in range(2):
        r = random.Random(seed)
        rosters.append(fuzz_roster(r, 257, 65, review_rooms=4))
    (plain, users, records), (relayed, _, _) = rosters
    bs, csenders = fuzz_broadcasts(rng, 257, records, counts)
    record = [rm is not None and rm < 4 and k % 3 == 0 for k, (_, rm, _, _, _) in enumerate(bs)]
    bad = []
    rl = relayed.relay_many(bs, clone_sender=csenders)
    bad += [f"plan: {x}" for x in plan_differences(rl.plan, relayed.plan_many(bs))]
    rl2 = relayed.relay_many(bs, record=record, clone_sender=csenders)
    bad += [f"recording plan: {x}" for x in plan_differences(rl2.plan, plain.plan_many(bs, record=record))]
    a, b = relayed.review_many([0, 1, 2, 3]), plain.review_many([0, 1, 2, 3])
    if any(a.lines(q) != b.lines(q) or a.chunks(q, c) != b.chunks(q, c) for q in range(4) for c in (0, 1)):
        bad.append("the rings differ after recording")
    recorded = sum(len(a.lines(q)) for q in range(4))
    with_relays = [k for k in range(len(bs)) if len(rl.relays(k))]
    without = [k for k in range(len(bs)) if not len(rl.relays(k))]
    for k in without:
        if (rl.relay_text(k), rl.relay_chunks(k, 0), rl.relay_chunks(k, 1), rl.owners(k).tolist()) != (b"", [], [], []) \
                or rl.variant_sizes[k].tolist() != [0, 0] or rl.write_counts[k].tolist() != [0, 0] or rl.text_sizes[k] != -1:
            bad.append(f"broadcast {k} relays nothing, but its relay fields are not empty")
    own = relayed.plan_many([(rl.relay_text(k), None, None, 0, 0) for k in with_relays])
    for i, k in enumerate(with_relays):
        for c in (0, 1):
            if rl.relay_chunks(k, c) != own.chunks(i, c):
                bad.append(f"relay variant ({k}, {c}) is not plan_many's of the relay text")
    plain.close()
    relayed.close()
    return {"with_relays": len(with_relays), "without": len(without), "recorded_lines": recorded, "n_bad": len(bad),
            "first_bad": bad[:2]}


def digest(rl: device.Relay) -> str:
    h = hashlib.sha256()
    h.update(rl.relay_bits.tobytes() + rl.plan.admitted_bits.tobytes())
    for k in range(len(rl.relay_bits)):
        for c in (0, 1):
            h.update(rl.relay_text(k) + bytes([0]) + b"".join(rl.relay_chunks(k, c)) + bytes(len(x) % 251 for x in rl.relay_chunks(k, c)))
            h.update(b"".join(rl.plan.chunks(k, c)))
    return h.hexdigest()


def determinism_part(seed: int) -> dict:
    out = []
    for _ in range(2):
        rng = random.Random(seed)
        roster, users, records = fuzz_roster(rng, 257, 257)
        bs, csenders = fuzz_broadcasts(rng, 257, records, new_counts())
        out.append([digest(roster.relay_many(bs, clone_sender=csenders)), digest(roster.relay_many(bs, clone_sender=csenders))])
        roster.close()
    return {"same_on_a_second_call": out[0][0] == out[0][1], "same_on_a_second_roster": out[0] == out[1]}


def all_other_calls(roster: device.Roster) -> dict:
    """other_calls of tests/device_look_child.py, and a look_many."""
    out = other_calls(roster)
    lk = roster.look_many([0, 1, 2])
    out["look"] = [[hashlib.sha256(b"\0".join(lk.chunks(k))).hexdigest() for k in range(3)], lk.members(0).tolist()[:8],
                   copies(lk.timing)]
    return out


def nothing_else_moved_part() -> dict:
    cap, nclones = 300, 70

    def build(clones):
        r = device.Roster(cap, review_rooms=2, look_rooms=len(ROOM_NAMES), clones=clones)
        r.update(list(range(cap)), room=[j % 2 for j in range(cap)], colour=[j % 3 == 0 for j in range(cap)],
                 name=[b"U%d" % j for j in range(cap)], level=2)
        r.update([0, 1], name=[b"Alice", b"Bobby"])
        r.set_rooms(list(range(len(ROOM_NAMES))), name=list(ROOM_NAMES), desc=b"A room.\n")
        return r

    fresh, cloned = build(0), build(nclones)
    cloned.set_clones(list(range(nclones)), owner=[c % cap for c in range(nclones)], room=[c % 2 for c in range(nclones)])
    out = {"capacity": cap, "clones": nclones, "look_rooms": len(ROOM_NAMES), "fresh": all_other_calls(fresh),
           "with_clones": all_other_calls(cloned)}
    bs = [(b"hello ~FRroom~RS\n", 0, 1, 0, 3), (b"to all\n", None, None, 1, 4), (b"a shit line\n", 1, None, 0, 6)]
    out["text_bytes"], out["broadcasts"] = sum(len(b[0]) for b in bs), len(bs)
    h = {}
    rl = cloned.relay_many(bs)
    h["first"] = rl.timing["h2d_bytes"]
    out["timing_keys"] = [sorted(rl.timing), sorted(rl.plan.timing), sorted(cloned.plan_many(bs).timing)]
    out["relays"] = [len(rl.relays(k)) for k in range(len(bs))]
    h["clean"] = [cloned.relay_many(bs).timing["h2d_bytes"] for _ in range(2)]
    h["plan_clean"] = cloned.plan_many(bs).timing["h2d_bytes"]
    cloned.set_clones(3, hear=SWEARS)
    h["after_set_clones"] = cloned.relay_many(bs).timing["h2d_bytes"]
    for r in (cloned, fresh):                                           # what the slots and the rooms see, both rosters see
        r.set_rooms(1, name=b"renamed")
    h["after_a_new_name"] = cloned.relay_many(bs).timing["h2d_bytes"]
    for r in (cloned, fresh):
        r.set_rooms(1, topic=b"a topic is no name")
    h["after_set_rooms_of_no_name"] = cloned.relay_many(bs).timing["h2d_bytes"]
    for r in (cloned, fresh):
        r.update(5, ignall=1)
    h["after_update"] = cloned.relay_many(bs).timing["h2d_bytes"]
    h["clean_again"] = cloned.relay_many(bs).timing["h2d_bytes"]
    for r in (cloned, fresh):
        r.update(5, ignall=0)
        r.set_rooms(1, name=ROOM_NAMES[1], topic=b"")
    cloned.relay_many(bs)
    out["relay_h2d"] = h
    out["after_relaying"] = all_other_calls(cloned)                     # and the other calls still answer alike
    out["fresh_again"] = all_other_calls(fresh)
    fresh.close()
    cloned.close()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261)
    args = ap.parse_args()
    if device.device_count() < 1:
        print("no GPU visible", file=sys.stderr)
        return 3
    res = {"fuzz": fuzz_part(args.seed), "contract": contract_part(args.seed + 1),
           "determinism": determinism_part(args.seed + 2), "moved": nothing_else_moved_part()}
    print("DEVICE_RELAY " + json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
