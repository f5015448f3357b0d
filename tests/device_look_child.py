"""The device work of tests/test_device_look.py, in a short-lived child process of its own, and the CPU model the host
tier of that module shares with it.

As tests/device_tell_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_LOOK {...}``).  ``look`` is the Python model of ``look()`` (nuts333.c:3942-4004), built from the
reference's format strings: the strings of its ``write_user`` calls, in order.  ``replay_looks`` runs a recorded session
of tests/golden: accounts are seated as they log in, the commands that change what a later look shows are applied, and
every recv string that holds a look is compared with the answer for that looker.

    python tests/device_look_child.py [--seed S]
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

from device_input_child import COMMAND, dispatch  # noqa: E402
from device_tell_child import new_user, word_1  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402
from nuts333_amd.provision import DEFAULT_ROOMS  # noqa: E402

#: the sessions the replay covers: ``rooms`` and eleven more, all recorded with the default rooms
GOLDEN = ("rooms", "prompts", "errors", "filters", "afk_bcast", "speech_colour_off", "speech_colour_mixed", "markup",
          "review", "swearing", "framing", "long_motd")
LOOK_MARK = "Access is "
CAPACITIES = (1, 63, 64, 65, 255, 256, 257, 1000)
LOOKERS_PER_CALL = 64
SPECIAL_SLOTS = (0, 63, 64, 255, 256)
ACCESS_WORDS = {device.PUBLIC: b"set to ~FGPUBLIC~RS", device.PRIVATE: b"set to ~FRPRIVATE~RS",
                device.FIXED_PUBLIC: b"~FRfixed~RS to ~FGPUBLIC~RS", device.FIXED_PRIVATE: b"~FRfixed~RS to ~FRPRIVATE~RS"}
#: descriptions at the edges: empty, all newlines, all colour commands, escapes, a slash before the line's ~RS, high bytes
WORST_DESCS = (b"", b"\n" * 30, b"~FR" * 10, b"/~" * 15, b"x" * 29 + b"/", b"~" * 30, b"\xe9\xff high \x80", b"is a user",
               b"~FR/", b"/" * 30)
WORST_NAMES = (b"A", b"Abcdefghijkl", b"\n" * 12, b"~FR~FG~FB~FT", b"/~/~/~/~/~/~", b"~" * 12, b"\xe9" * 12)


# ------------------------------------------------------------------ the model
def new_room(name=b"room", **fields) -> dict:
    return {"name": name, "access": device.PUBLIC, "desc": b"", "links": [], "topic": b"", "mesg_cnt": 0, "netlink": None,
            **fields}


def members(users: dict, slot: int) -> list:
    """The slots look() lists for users[slot] (c:3976-3978), in list order; a slot without a name is not a user."""
    u = users[slot]
    return [j for j in sorted(users) if j != slot and users[j]["room"] == u["room"] and users[j]["name"]
            and (users[j]["vis"] or users[j]["level"] <= u["level"])]


def member_line(m: dict) -> bytes:
    afk = b"~BR(AFK)" if m["afk"] else b""
    if not m["vis"]:
        return b"     ~FR*~RS%s %s~RS  %s\n" % (m["name"], m["desc"], afk)       # c:3981
    return b"      %s %s~RS  %s\n" % (m["name"], m["desc"], afk)                  # c:3982


def look(users: dict, rooms, slot: int) -> list:
    """The strings look() hands to write_user for users[slot], in order."""
    rm = rooms[users[slot]["room"]]
    out = [b"\n~FTRoom: %s%s\n\n" % (b"~FR" if rm["access"] & 1 else b"~FG", rm["name"]), rm["desc"]]
    text = b"\n~FTExits are:"
    for l in rm["links"]:
        text += b"  %s%s" % (b"~FR" if rooms[l]["access"] & 1 else b"~FG", rooms[l]["name"])
    if rm["netlink"]:
        text += b"  %s%s*" % (b"~FR" if rm["netlink"][1] else b"~FG", rm["netlink"][0])
    elif not rm["links"]:
        text = b"\n~FTThere are no exits."
    out.append(text + b"\n\n")
    listed = members(users, slot)
    if listed:
        out.append(b"~FTYou can see:\n")
        out += [member_line(users[j]) for j in listed]
    else:
        out.append(b"~FTYou are all alone here.\n")
    out.append(b"\n")
    out.append(b"Access is %s and there are ~OL~FM%d~RS messages on the board.\n" % (ACCESS_WORDS[rm["access"]], rm["mesg_cnt"]))
    out.append(b"Current topic: %s\n" % rm["topic"] if rm["topic"] else b"No topic has been set yet.\n")
    return out


def model_chunks(users: dict, rooms, slot: int) -> list:
    c = int(users[slot]["colour"])
    return [ch for s in look(users, rooms, slot) for ch in nuts_path.chunks(s, c)]


# ------------------------------------------------------------------ a roster and its model
FIELDS = ("room", "login", "colour", "name", "vis", "level", "afk", "desc")


def look_user(slot: int, **fields) -> dict:
    return new_user(slot, **{"desc": b"", "prompt": 0, **fields})


def seat(roster: device.Roster, u: dict) -> None:
    fields = {f: u[f] for f in FIELDS if f != "name"}
    fields["afk"] = int(bool(u["afk"]))
    if u["name"]:
        fields["name"] = u["name"]
    roster.update(u["slot"], **fields)


def set_rooms(roster: device.Roster, rooms) -> None:
    ids = list(range(len(rooms)))
    roster.set_rooms(ids, **{f: [rooms[i][f] for i in ids] for f in ("name", "access", "desc", "links", "topic", "mesg_cnt",
                                                                      "netlink")})


def default_rooms() -> list:
    """The rooms every session of GOLDEN was recorded with (nuts333_amd.provision.DEFAULT_ROOMS), as parse_rooms reads
    them (nuts333.c:928-931): no netlink is UP in these sessions."""
    label = {r.label: i for i, r in enumerate(DEFAULT_ROOMS)}
    access = {"": device.PUBLIC, "BOTH": device.PUBLIC, "PUB": device.FIXED_PUBLIC, "PRIV": device.FIXED_PRIVATE}
    return [new_room(r.name.encode(), access=access[r.access], desc=r.description.encode(), links=[label[l] for l in r.links])
            for r in DEFAULT_ROOMS]


def model_answer(roster, users, rooms, slot) -> bytes:
    return b"".join(model_chunks(users, rooms, slot))


def golden_looks(name: str) -> int:
    """The recv strings of session ``name`` that hold a look."""
    doc = json.loads((REPO / "tests" / "golden" / f"{name}.json").read_text())
    return sum(LOOK_MARK in r for s in doc["steps"] for r in s.get("recv", {}).values())


def replay_looks(name: str, answer) -> dict:
    """Session ``name`` of tests/golden: accounts are seated in slots in login order, in room 0, with the account's desc;
    .quit, .vis / .invis, .afk (and what user_input does for an AFK user), .colour, .desc, .topic, .mode and .prompt are
    applied, and a .go that succeeded -- its actor's bytes begin with a look -- moves the user to the room its word
    names by prefix, as get_room matches.  Every recv string that holds ``Access is `` is a look of that step's actor:
    ``answer(roster, users, rooms, slot)`` must occur in it as one run -- from its first byte for a .look or a .go,
    anywhere for a login -- and nothing may follow it but the prompt of a user who has one or is in command mode (a
    single line), except after a .go."""
    lib = nuts_path.lib()
    doc = json.loads((REPO / "tests" / "golden" / f"{name}.json").read_text())
    accounts = {}
    for group in doc["accounts"]:
        for acc in (group if isinstance(group, list) else [group]):
            accounts[acc["name"]] = acc
    rooms = default_rooms()
    roster = device.Roster(8, look_rooms=len(rooms))
    set_rooms(roster, rooms)
    seats, users = {}, {}
    res = {"compared": 0, "mismatches": [], "kinds": {}}

    def compare(step, kind):
        actor = step["actor"]
        for who, text in step["recv"].items():
            if LOOK_MARK not in text:
                continue
            res["compared"] += 1
            res["kinds"][kind] = res["kinds"].get(kind, 0) + 1
            u = users[seats[actor]]
            for s in users.values():
                seat(roster, s)
            set_rooms(roster, rooms)
            got, want = answer(roster, users, rooms, u["slot"]), text.encode("latin-1")
            at = want.find(got)
            rest = want[at + len(got):] if at >= 0 else b""
            ok = who == actor and at >= 0 and (kind == "login" or at == 0)
            if kind != "go":
                ok = ok and (rest == b"" or bool((u["prompt"] or u["command_mode"]) and re.fullmatch(rb"[^\n]*(\n\r(\x1b\[0m)?)?", rest)))
            if not ok:
                res["mismatches"].append({"step": step.get("send", step["op"]), "actor": who, "at": at,
                                          "got": got.decode("latin-1"), "want": text})

    for step in doc["steps"]:
        if step["op"] == "login":
            acc, slot = accounts[step["name"]], len(seats)
            seats[step["actor"]] = slot
            users[slot] = look_user(slot, name=acc["name"].encode("latin-1"), command_mode=int(bool(acc["command_mode"])),
                                    level=int(acc["level"]), colour=int(bool(acc["colour"])), desc=acc["desc"].encode("latin-1"),
                                    prompt=int(bool(acc["prompt"])))
            compare(step, "login")
        elif step["op"] == "line":
            data = step["send"].encode("latin-1") + b"\n"
            u = users[seats[step["actor"]]]
            d = dispatch(u, data)
            if u["afk"]:                                                # user_input, nuts333.c:211s
                if u["afk"] == 2:                                       # locked: the line is the password, or nothing
                    if "Session unlocked" in step["recv"].get(step["actor"], ""):
                        u.update(afk=0)
                    continue
                u.update(afk=0)
            if d["kind"] != COMMAND:
                continue
            what = lib.np_command_name(d["com"]).decode()
            inpstr = data[d["start"]:d["start"] + d["size"]]
            if what in ("vis", "invis"):
                u["vis"] = int(what == "vis")
            elif what == "colour":
                u["colour"] ^= 1
            elif what == "prompt":
                u["prompt"] ^= 1
            elif what == "mode":
                u["command_mode"] ^= 1
            elif what == "quit":
                u["room"] = None
            elif what == "afk":                                         # afk(), nuts333.c:7409-7454
                lock = d["word_count"] > 1 and word_1(inpstr) == b"lock"
                mesg = lib.np_remove_first(inpstr) if lock else inpstr
                if not (d["word_count"] > 1 and len(mesg) > device.AFK_MESG_LEN):
                    u["afk"] = 2 if lock else 1
            elif what == "desc":                                        # set_desc, nuts333.c:5062-5081
                if d["word_count"] > 1 and b"(CLONE)" not in word_1(inpstr) and len(inpstr) <= device.USER_DESC_LEN:
                    u["desc"] = inpstr
            elif what == "topic":                                       # set_topic, nuts333.c:5226-5250
                if d["word_count"] > 1 and len(inpstr) <= device.TOPIC_LEN:
                    rooms[u["room"]]["topic"] = inpstr
            elif what == "go":
                if LOOK_MARK in step["recv"].get(step["actor"], ""):
                    word = word_1(inpstr)
                    u["room"] = next(i for i, rm in enumerate(rooms) if rm["name"].startswith(word))    # get_room, c:2412
                    compare(step, "go")
            elif what == "look":
                compare(step, "look")
    roster.close()
    return res


# ------------------------------------------------------------------ seeded rosters
def fuzz_rooms(rng: random.Random) -> list:
    """Five rooms: every access value, 0 and 10 links, links to private rooms, a netlink in, out and alone, no exits at
    all, empty and 60-byte topics, mesg_cnt 0 and 2^31 - 1, and the descriptions at the transducer's edges."""
    descs = [b"\n" * 810, b"~FR" * 270, b"/~" * 405, b"", b"A room.\nWith ~OLtwo~RS lines and a slash/\n"]
    rng.shuffle(descs)
    return [new_room(b"R" * 20, access=device.FIXED_PUBLIC, desc=descs[0], links=[1, 2, 3, 4, 1, 2, 3, 4, 1, 2],
                     topic=b"t" * 60, mesg_cnt=2**31 - 1, netlink=(b"s" * 80, True)),
            new_room(b"alone", access=device.PRIVATE, desc=descs[1], netlink=(b"peer2", False)),
            new_room(b"pair", access=device.FIXED_PRIVATE, desc=descs[2], mesg_cnt=rng.randrange(1000)),
            new_room(b"~FRred/", access=device.PUBLIC, desc=descs[3], links=[2, 1], topic=b"~OLbold~RS /~FR \xe9",
                     netlink=(b"in", True), mesg_cnt=10),
            new_room(b"e", access=device.PUBLIC, desc=descs[4], links=[0], mesg_cnt=7)]


def fuzz_roster(rng: random.Random, cap: int, **kw):
    """A roster of ``cap`` slots over five rooms, populated unevenly: room 0 holds most (more than 256 at capacity 1000),
    room 1 one user alone, room 2 a pair; users planted at slots 0, 63, 64, 255, 256 and cap - 1 of room 0."""
    rooms = fuzz_rooms(rng)
    roster = device.Roster(cap, look_rooms=len(rooms), **kw)
    set_rooms(roster, rooms)
    users = {}
    for j in range(cap):
        x = rng.random()
        users[j] = look_user(j, room=0 if x < 0.62 else 3 if x < 0.8 else 4 if x < 0.94 else None,
                             name=rng.choice(WORST_NAMES + (b"Bobby", b"Q%d" % j)) if rng.random() < 0.9 else None,
                             vis=int(rng.random() < 0.7), level=rng.randrange(5), afk=int(rng.random() < 0.15),
                             colour=rng.randrange(2), login=int(rng.random() < 0.1), desc=rng.choice(WORST_DESCS))
    for s in sorted({s for s in SPECIAL_SLOTS + (cap - 1,) if 0 <= s < cap}):
        users[s].update(room=0, name=b"P%011d" % s, vis=1)
    if cap >= 8:
        users[1].update(room=1, name=b"Alone")
        users[2].update(room=2, name=b"Pair1", vis=1)
        users[3].update(room=2, name=b"Pair2", vis=0, level=4)
        users[4].update(room=0, name=None)                              # a slot without a name is no user
    for u in users.values():
        seat(roster, u)
    return roster, users, rooms


def look_differences(users: dict, rooms, slots, lk: device.Look, counts: dict) -> list:
    bad = []
    for k, slot in enumerate(slots):
        want, listed = model_chunks(users, rooms, slot), members(users, slot)
        u = users[slot]
        counts["access"].add(rooms[u["room"]]["access"])
        counts["most_members"] = max(counts["most_members"], len(listed))
        counts["alone"] += not listed
        counts["afk"] += sum(bool(users[j]["afk"]) for j in listed)
        counts["hidden_by_level"] += sum(1 for j, m in users.items() if j != slot and m["room"] == u["room"] and m["name"]
                                         and not m["vis"] and m["level"] > u["level"])
        counts["colours"].add(int(u["colour"]))
        got = lk.chunks(k)
        where = {"look": k, "slot": slot, "room": u["room"], "colour": u["colour"]}
        if lk.members(k).tolist() != listed:
            bad.append({**where, "what": "members", "device": lk.members(k).tolist()[:20], "model": listed[:20]})
        elif got != want:
            i = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            bad.append({**where, "what": "chunks", "first": i, "device": [len(x) for x in got][:12], "model": [len(x) for x in want][:12],
                        "device_chunk": got[i][:60].decode("latin-1") if i < len(got) else None,
                        "model_chunk": want[i][:60].decode("latin-1") if i < len(want) else None})
        elif lk.output(k) != b"".join(got):
            bad.append({**where, "what": "output"})
    return bad


def new_counts() -> dict:
    return {"access": set(), "most_members": 0, "alone": 0, "afk": 0, "hidden_by_level": 0, "colours": set()}


def pick_lookers(rng: random.Random, users: dict, cap: int) -> list:
    seated = [j for j, u in users.items() if u["room"] is not None]
    must = [s for s in (0, 1, 2, 3, cap - 1) if s < cap and users[s]["room"] is not None]
    slots = must + [rng.choice(seated) for _ in range(LOOKERS_PER_CALL - len(must) - 1)]
    return slots + [slots[0]]                                           # duplicates are allowed


# ------------------------------------------------------------------ the parts of the device run
def fuzz_part(seed: int) -> dict:
    rng = random.Random(seed)
    counts, bad, calls, looks = new_counts(), [], 0, 0
    for cap in CAPACITIES:
        roster, users, rooms = fuzz_roster(rng, cap)
        for _ in range(2):
            slots = pick_lookers(rng, users, cap)
            lk = roster.look_many(slots)
            bad += look_differences(users, rooms, slots, lk, counts)
            calls += 1
            looks += len(slots)
            j = rng.randrange(cap)                                      # something changes between the calls
            users[j].update(desc=rng.choice(WORST_DESCS), afk=rng.randrange(2))
            seat(roster, users[j])
        roster.close()
    return {"capacities": list(CAPACITIES), "calls": calls, "looks": looks, "access": sorted(counts["access"]),
            "most_members": counts["most_members"], "alone": counts["alone"], "afk": counts["afk"],
            "hidden_by_level": counts["hidden_by_level"], "colours": sorted(counts["colours"]), "n_bad": len(bad),
            "first_bad": bad[:1]}


def contract_part(seed: int) -> dict:
    """Every text of a Look is the model's string, and its variants are plan_many's of that string."""
    rng = random.Random(seed)
    roster, users, rooms = fuzz_roster(rng, 257)
    slots = pick_lookers(rng, users, 257)
    lk = roster.look_many(slots)
    bad, checked = [], 0
    numbers = sorted({t for k in range(len(slots)) for t in lk.text_numbers(k)})
    strings = {}
    for k, slot in enumerate(slots):
        for t, s in zip(lk.text_numbers(k), look(users, rooms, slot)):
            strings[t] = s
    plan = roster.plan_many([(strings[t], None, None, 0, 0) for t in numbers])
    for i, t in enumerate(numbers):
        checked += 1
        if lk.text(t) != strings[t]:
            bad.append({"text": t, "what": "text", "device": lk.text(t)[:60].decode("latin-1")})
        for c in (0, 1):
            if lk.text_chunks(t, c) != plan.chunks(i, c):
                bad.append({"text": t, "what": "variant", "colour": c})
    roster.close()
    return {"checked": checked, "room_texts": sum(t < 5 * len(lk.rooms) for t in numbers), "n_bad": len(bad), "first_bad": bad[:1]}


def digest(lk: device.Look) -> str:
    h = hashlib.sha256()
    for k in range(len(lk.slots)):
        h.update(b"".join(lk.chunks(k)) + bytes([0]) + lk.members(k).tobytes() + bytes(len(c) % 251 for c in lk.chunks(k)))
    return h.hexdigest()


def determinism_part(seed: int) -> dict:
    out = []
    for _ in range(2):
        rng = random.Random(seed)
        roster, users, rooms = fuzz_roster(rng, 1000)
        slots = pick_lookers(rng, users, 1000)
        out.append([digest(roster.look_many(slots)), digest(roster.look_many(slots))])
        roster.close()
    return {"same_on_a_second_call": out[0][0] == out[0][1], "same_on_a_second_roster": out[0] == out[1]}


def plan_digest(p: device.Plan) -> list:
    k = len(p.variant_sizes)
    return [[[c.hex() for c in p.chunks(i, c)] for c in (0, 1)] for i in range(k)] + [p.admitted_bits.tolist()]


def copies(t: dict) -> list:
    return [t["h2d_bytes"], t["d2h_bytes"]]


def other_calls(roster: device.Roster) -> dict:
    """One call of each other kind, with what it returned and what it copied."""
    out = {}
    p = roster.plan_many([(b"hello ~FRroom~RS\n", 0, 1, 0, 3), (b"to all\n", None, None, 1, 4)], record=[True, False])
    out["plan"] = [plan_digest(p), copies(p.timing)]
    sp = roster.speak_many([(0, device.COM_SAY, b"hi there?", 2), (1, device.COM_SHOUT, b"loud", 2)])
    out["speak"] = [sp.outcome.tolist(), plan_digest(sp.room), plan_digest(sp.reply), copies(sp.timing)]
    inp = roster.input_many([(0, b".say x y\n"), (1, b"plain words\n"), (0, b".bogus\n")])
    out["input"] = [inp.kind.tolist(), inp.com.tolist(), plan_digest(inp.speech.room), plan_digest(inp.speech.reply),
                    copies(inp.timing)]
    pv = roster.tell_many([(0, device.COM_TELL, b"bobby psst", 3), (1, device.COM_PEMOTE, b"alice waves", 3)])
    out["tell"] = [pv.outcome.tolist(), pv.target.tolist(), plan_digest(pv.told), plan_digest(pv.reply), copies(pv.timing)]
    rv = roster.review_many([0, 1])
    out["review"] = [[[c.hex() for c in rv.chunks(q, c)] for c in (0, 1)] for q in range(2)] + [copies(rv.timing)]
    return out


def nothing_else_moved_part() -> dict:
    cap = 300
    rooms = fuzz_rooms(random.Random(5))

    def build(look_rooms):
        r = device.Roster(cap, review_rooms=2, look_rooms=look_rooms)
        r.update(list(range(cap)), room=[j % 2 for j in range(cap)], colour=[j % 3 == 0 for j in range(cap)],
                 name=[b"U%d" % j for j in range(cap)], level=2)
        r.update([0, 1], name=[b"Alice", b"Bobby"])
        return r

    fresh, looked = build(0), build(len(rooms))
    set_rooms(looked, rooms)
    looked.update(list(range(cap)), desc=[WORST_DESCS[j % len(WORST_DESCS)] for j in range(cap)])
    out = {"capacity": cap, "look_rooms": len(rooms), "fresh": other_calls(fresh), "with_look_rooms": other_calls(looked)}
    h = {}
    h["first"] = looked.look_many([0, 1, 2]).timing["h2d_bytes"]
    h["clean"] = [looked.look_many([0, 1, 2]).timing["h2d_bytes"] for _ in range(2)]
    looked.update(7, desc=b"changed")
    h["after_desc_update"] = looked.look_many([0, 1, 2]).timing["h2d_bytes"]
    looked.set_rooms(1, topic=b"new topic")
    h["after_set_rooms"] = looked.look_many([0, 1, 2]).timing["h2d_bytes"]
    h["clean_again"] = looked.look_many([0, 1, 2]).timing["h2d_bytes"]
    out["look_h2d"] = h
    out["after_looking"] = other_calls(looked)                          # and the other calls still answer alike
    out["fresh_again"] = other_calls(fresh)
    fresh.close()
    looked.close()
    return out


def golden_part() -> dict:
    out = {}
    for name in GOLDEN:
        vs_model = []

        def answer(roster, users, rooms, slot):
            got = roster.look_many([slot])
            if got.chunks(0) != model_chunks(users, rooms, slot) or got.members(0).tolist() != members(users, slot):
                vs_model.append(slot)
            return got.output(0)

        res = replay_looks(name, answer)
        out[name] = {"compared": res["compared"], "mismatches": res["mismatches"][:2], "n_bad_vs_model": len(vs_model),
                     "kinds": res["kinds"]}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20260)
    args = ap.parse_args()
    if device.device_count() < 1:
        print("no GPU visible", file=sys.stderr)
        return 3
    res = {"golden": golden_part(), "fuzz": fuzz_part(args.seed), "contract": contract_part(args.seed + 1),
           "determinism": determinism_part(args.seed + 2), "moved": nothing_else_moved_part()}
    print("DEVICE_LOOK " + json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
