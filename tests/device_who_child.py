"""The device work of tests/test_device_who.py, in a short-lived child process of its own, and the CPU model the host
tier of that module shares with it.

As tests/device_look_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_WHO {...}``).  ``who`` is the Python model of ``who(user, 0)`` (nuts333.c:4792-4856), built from
the reference's format strings: the strings of its ``write_user`` calls, in order.  ``colour_com_count`` restates
c:2563-2583, which is not the transducer's count.  ``replay_whos`` runs the recorded session
tests/golden/reference_only/who.json: accounts are seated as they log in, ``.go``, ``.invis`` and ``.afk`` are applied,
and the bytes of every ``.who`` -- and of the ``who`` typed at the name prompt -- are compared with the answer.

    python tests/device_who_child.py [--seed S]
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

from device_look_child import copies, default_rooms, look_user, new_room, other_calls, set_rooms  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402

GOLDEN = REPO / "tests" / "golden" / "reference_only" / "who.json"
DATE = b"DATE"
CAPACITIES = (1, 64, 65, 257, 1025)
LOOKERS_PER_CALL = 8
#: the listed-user counts the fuzz must land on: the bitmap word, wave and block edges
EDGES = (0, 1, 31, 32, 33, 63, 64, 65, 256, 257)
#: colcom[] in its order (nuts333.h:249-255)
COLCOM = (b"RS", b"OL", b"UL", b"LI", b"RV", b"FK", b"FR", b"FG", b"FY", b"FB", b"FM", b"FT", b"FW", b"BK", b"BR", b"BG", b"BY",
          b"BB", b"BM", b"BT", b"BW")
#: descriptions that colour_com_count and the transducer count differently, and the plain edges
QUIRK_DESCS = (b"~FR", b"~FBK", b"~OLI", b"~FBBM", b"~FBBT", b"~~FR", b"ends in ~", b"ends in ~F", b"~FBBM" * 6, b"", b"is a user",
               b"x" * 30, b"~FR/", b"\n~RS\n", b"~ULI~RVS", b"\xe9\xff high")
QUIRK_NAMES = (b"A", b"Abcdefghijkl", b"~FBBM~OLI~FR", b"~FBBM~FBBM~~", b"Bobby")
FIELDS = ("room", "login", "colour", "name", "vis", "level", "afk", "desc", "last_login", "away")


# ------------------------------------------------------------------ the model
def colour_com_count(s: bytes) -> int:
    """c:2563-2583: behind a ``~`` the table is walked once, and a match counts, advances ONE byte and lets the walk go on
    with the entries after it at the new place."""
    at, cnt = 0, 0
    while at < len(s):
        if s[at] != ord("~"):
            at += 1
            continue
        at += 1
        for code in COLCOM:
            if s[at:at + 2] == code:
                cnt += 1
                at += 1
    return cnt


def who_user(slot: int, **fields) -> dict:
    return look_user(slot, **{"last_login": 0, "away": None, **fields})


def listed(users: dict) -> list:
    """The slots who() counts into ``total`` (c:4808-4827), in list order: a slot without a name is no user."""
    return [j for j in sorted(users) if users[j]["name"] and not users[j]["login"]]


def shown(users: dict, slot: int) -> list:
    u = users[slot]
    return [j for j in listed(users) if users[j]["vis"] or users[j]["level"] <= u["level"]]        # c:4832-4835


def who_line(m: dict, rooms, now: int) -> bytes:
    line = b"  %s %s~RS" % (m["name"], m["desc"])                                                    # c:4838
    if not m["vis"]:
        line = b"*" + line[1:]
    rname = rooms[m["room"]]["name"] if m["room"] is not None else b"@" + rooms[m["away"]]["netlink"][0]   # c:4841
    d = now - m["last_login"]
    mins = -(-d // 60) if d < 0 else d // 60                                                         # C's (int)x / 60
    text = b"%-*s : %-4s : %-12s : %d mins." % (40 + 3 * colour_com_count(line), line, device.LEVEL_NAMES[m["level"]], rname, mins)
    return text + (b"~BR(AFK)\n" if m["afk"] else b"\n")


def who(users: dict, rooms, slot: int, now: int, date: bytes) -> list:
    """The strings who(user, 0) hands to write_user for users[slot], in order."""
    u = users[slot]
    out = [(b"\n*** Current users %s ***\n\n" if u["login"] else b"\n~BB*** Current users %s ***\n\n") % date]
    out += [who_line(users[j], rooms, now) for j in shown(users, slot)]
    total = listed(users)
    invis = sum(not users[j]["vis"] for j in total)
    out.append(b"\nThere are %d visible, %d invisible, %d remote users.\nTotal of %d users" % (len(total) - invis, invis, 0, len(total)))
    out.append(b".\n\n")
    return out


def model_chunks(users: dict, rooms, slot: int, now: int, date: bytes) -> list:
    c = int(users[slot]["colour"])
    return [ch for s in who(users, rooms, slot, now, date) for ch in nuts_path.chunks(s, c)]


def seat(roster: device.Roster, u: dict) -> None:
    fields = {f: u[f] for f in FIELDS if f != "name"}
    fields["afk"] = int(bool(u["afk"]))
    if u["name"]:
        fields["name"] = u["name"]
    roster.update(u["slot"], **fields)


# ------------------------------------------------------------------ the recorded session
def golden_whos() -> int:
    doc = json.loads(GOLDEN.read_text())
    return sum(s.get("send") in (".who", "who") for s in doc["steps"])


def replay_whos(answer) -> dict:
    """tests/golden/reference_only/who.json: a client gets the next slot as it connects, at the name prompt (``login``
    set, no name); its login seats the account there, in room 0.  A ``.go`` that succeeded moves its actor, ``.invis``
    and ``.afk`` mark it.  ``answer(users, rooms, slot, now, date)`` must be, byte for byte, what the actor of a ``.who``
    received; a ``who`` at the name prompt is followed by the next name prompt.  ``mins`` is 0 throughout the session:
    every login is seconds old."""
    doc = json.loads(GOLDEN.read_text())
    accounts = {a["name"]: a for a in doc["accounts"][0]}
    rooms = default_rooms()
    seats, users = {}, {}
    res = {"compared": 0, "mismatches": [], "kinds": {}}
    for step in doc["steps"]:
        actor, send = step["actor"], step.get("send", "")
        if step["op"] == "connect":
            seats[actor] = len(seats)
            users[seats[actor]] = who_user(seats[actor], room=None, login=1, level=0)     # create_user: NEW
        elif step["op"] == "login":
            acc = accounts[step["name"]]
            users[seats[actor]].update(room=0, login=0, name=acc["name"].encode("latin-1"), level=int(acc["level"]),
                                       colour=int(bool(acc["colour"])), desc=acc["desc"].encode("latin-1"), last_login=1000)
        elif send.startswith(".go ") and "Access is " in step["recv"].get(actor, ""):
            users[seats[actor]]["room"] = next(i for i, rm in enumerate(rooms) if rm["name"].startswith(send[4:].encode()))
        elif send == ".invis":
            users[seats[actor]]["vis"] = 0
        elif send == ".afk":
            users[seats[actor]]["afk"] = 1
        elif send in (".who", "who"):
            kind = "prompt" if send == "who" else "colour" if users[seats[actor]]["colour"] else "plain"
            res["compared"] += 1
            res["kinds"][kind] = res["kinds"].get(kind, 0) + 1
            got = answer(users, rooms, seats[actor], 1000, DATE) + (b"\n\rGive me a name: " if send == "who" else b"")
            want = step["recv"][actor].encode("latin-1")
            if got != want:
                res["mismatches"].append({"step": step.get("note", send), "actor": actor, "got": got.decode("latin-1"),
                                          "want": step["recv"][actor]})
    return res


# ------------------------------------------------------------------ seeded rosters
def fuzz_rooms() -> list:
    """Six rooms: a 20-byte name that overflows %-12s, a 12-byte one, short ones, and two with a netlink to be away over,
    one of them with an 80-byte service."""
    return [new_room(b"R" * 20), new_room(b"twelve_bytes"), new_room(b"e"), new_room(b"~FRred/", netlink=(b"in", True)),
            new_room(b"far", netlink=(b"s" * 80, False)), new_room(b"drive", netlink=(b"", True))]


def fuzz_roster(rng: random.Random, cap: int, want: int, now: int):
    """A roster of ``cap`` slots with exactly ``want`` listed users, the rest nameless, at login stage or both; users of
    all five levels, both colour bits, invisible ones, AFK ones, roomless ones away over a link, login times before and
    after ``now``."""
    rooms = fuzz_rooms()
    roster = device.Roster(cap, look_rooms=len(rooms))
    set_rooms(roster, rooms)
    chosen = set(rng.sample(range(cap), want))
    users = {}
    for j in range(cap):
        away = rng.random() < 0.12
        u = who_user(j, room=None if away else rng.randrange(len(rooms)), away=rng.choice((3, 4, 5)) if away else None,
                     name=rng.choice(QUIRK_NAMES + (b"Q%d" % j,)), vis=int(rng.random() < 0.7), level=rng.randrange(5),
                     afk=int(rng.random() < 0.15), colour=rng.randrange(2), desc=rng.choice(QUIRK_DESCS),
                     last_login=rng.choice((0, now, now + 61, now + 59, max(0, now - 3599), rng.randrange(2**31))))
        if j not in chosen:
            kind = rng.randrange(3)
            if kind != 0:
                u["login"] = 1
            if kind != 1:
                u["name"] = None
            if rng.random() < 0.5:
                u["room"], u["away"] = None, None                       # a slot that is no user needs no room
        users[j] = u
        seat(roster, u)
    assert len(listed(users)) == want
    return roster, users, rooms


def bits_of(users: dict, slots) -> list:
    order = listed(users)
    words = max(1, -(-len(order) // 32))
    out = np.zeros((len(slots), words), dtype=np.uint32)
    for k, slot in enumerate(slots):
        see = set(shown(users, slot))
        for l, j in enumerate(order):
            if j in see:
                out[k, l // 32] |= np.uint32(1 << (l % 32))
    return out.tolist()


def who_differences(users: dict, rooms, slots, now: int, date: bytes, w: device.Who, counts: dict) -> list:
    bad, order = [], listed(users)
    if w.line_slots.tolist() != order:
        bad.append({"what": "line_slots", "device": w.line_slots.tolist()[:20], "model": order[:20]})
    if w.shown.dtype != np.uint32 or w.shown.tolist() != bits_of(users, slots):
        bad.append({"what": "shown", "shape": list(w.shown.shape)})
    fixed = who(users, rooms, slots[0], now, date)
    strings = {device.WHO_HEAD_LOGIN: b"\n*** Current users %s ***\n\n" % date, device.WHO_HEAD: b"\n~BB*** Current users %s ***\n\n" % date,
               device.WHO_FOOT: fixed[-2], device.WHO_TAIL: fixed[-1]}
    strings.update({4 + l: who_line(users[j], rooms, now) for l, j in enumerate(order)})
    if len(w.text_sizes) != len(strings):
        bad.append({"what": "texts", "device": len(w.text_sizes), "model": len(strings)})
    for t, s in strings.items():
        if w.text(t) != s:
            bad.append({"what": "text", "text": t, "device": w.text(t).decode("latin-1"), "model": s.decode("latin-1")})
            break
        for c in (0, 1):
            ch = nuts_path.chunks(s, c)
            if w.text_chunks(t, c) != ch or w.write_sizes[t, c, :w.write_counts[t, c]].tolist() != [len(x) for x in ch]:
                bad.append({"what": "variant", "text": t, "colour": c})
                break
    for k, slot in enumerate(slots):
        u = users[slot]
        counts["levels"].add(int(u["level"]))
        counts["colours"].add(int(u["colour"]))
        counts["login_lookers"] += int(u["login"])
        counts["hidden_by_level"] += len(order) - len(shown(users, slot))
        want = model_chunks(users, rooms, slot, now, date)
        where = {"who": k, "slot": slot, "colour": u["colour"], "listed": len(order)}
        if [order[l] for l in w.lines(k)] != shown(users, slot):
            bad.append({**where, "what": "lines"})
        elif w.chunks(k) != want:
            bad.append({**where, "what": "chunks"})
        elif w.output(k) != b"".join(want):
            bad.append({**where, "what": "output"})
    counts["afk"] += sum(bool(users[j]["afk"]) for j in order)
    counts["away"] += sum(users[j]["room"] is None for j in order)
    counts["negative_mins"] += sum(users[j]["last_login"] > now + 60 for j in order)
    counts["quirk_counts"] |= {colour_com_count(b"  %s %s~RS" % (users[j]["name"], users[j]["desc"])) for j in order}
    return bad


def new_counts() -> dict:
    return {"levels": set(), "colours": set(), "login_lookers": 0, "hidden_by_level": 0, "afk": 0, "away": 0, "negative_mins": 0,
            "quirk_counts": set()}


def pick_lookers(rng: random.Random, cap: int) -> list:
    slots = [rng.randrange(cap) for _ in range(LOOKERS_PER_CALL - 1)]
    return slots + [slots[0]]                                           # duplicates are allowed


def cases() -> list:
    """(capacity, listed users): every edge in a roster it fills or nearly fills, and in a sparse one."""
    return [(1, 0), (1, 1), (64, 31), (64, 32), (64, 33), (64, 63), (64, 64), (65, 1), (65, 64), (65, 65), (257, 0), (257, 33),
            (257, 65), (257, 256), (257, 257), (1025, 64), (1025, 256), (1025, 257), (1025, 1025)]


def fuzz_part(seed: int) -> dict:
    rng = random.Random(seed)
    counts, bad, calls, seen = new_counts(), [], 0, set()
    now, date = 1_000_000, b"on Monday 19 October 2026 at 00:07"
    for cap, want in cases():
        roster, users, rooms = fuzz_roster(rng, cap, want, now)
        slots = pick_lookers(rng, cap)
        w = roster.who_many(slots, now=now, date=date)
        bad += [{"capacity": cap, **b} for b in who_differences(users, rooms, slots, now, date, w, counts)]
        seen.add(want)
        calls += 1
        roster.close()
    return {"capacities": sorted({c for c, _ in cases()}), "listed": sorted(seen), "calls": calls, "levels": sorted(counts["levels"]),
            "colours": sorted(counts["colours"]), "login_lookers": counts["login_lookers"], "hidden_by_level": counts["hidden_by_level"],
            "afk": counts["afk"], "away": counts["away"], "negative_mins": counts["negative_mins"],
            "quirk_counts": sorted(counts["quirk_counts"]), "dense": sum(n == c for c, n in cases()),
            "sparse": sum(0 < n <= c // 4 for c, n in cases()), "n_bad": len(bad), "first_bad": bad[:1]}


def worst_user(slot: int, **fields) -> dict:
    """The longest line: a 12-byte name, the 19-count description, away over an 80-byte service, the widest mins, AFK."""
    return who_user(slot, **{"name": b"Abcdefghijkl", "desc": b"~FBBM" * 6, "room": None, "away": 4, "last_login": 2**31 - 1, "afk": 1,
                             **fields})


def worst_part() -> dict:
    rooms = fuzz_rooms()
    users = {0: worst_user(0, colour=1), 1: worst_user(1, name=b"~FBBM~OLI~FR", vis=0), 2: worst_user(2, last_login=0)}
    out = {}
    for now in (0, 2**31 - 1):
        roster = device.Roster(3, look_rooms=len(rooms))
        set_rooms(roster, rooms)
        for u in users.values():
            seat(roster, u)
        w = roster.who_many([0, 1], now=now, date=b"d" * device.WHO_DATE_LEN)
        bad = who_differences(users, rooms, [0, 1], now, b"d" * device.WHO_DATE_LEN, w, new_counts())
        out[str(now)] = {"n_bad": len(bad), "first_bad": bad[:1], "longest": int(w.text_sizes.max()),
                         "most_bytes": int(w.variant_sizes[4:].max()), "most_writes": int(w.write_counts[4:].max())}
        roster.close()
    return out


def digest(w: device.Who) -> str:
    h = hashlib.sha256()
    for k in range(len(w.slots)):
        h.update(b"".join(w.chunks(k)) + bytes([0]) + w.shown[k].tobytes() + bytes(len(c) % 251 for c in w.chunks(k)))
    return h.hexdigest()


def determinism_part(seed: int) -> dict:
    out = []
    for _ in range(2):
        rng = random.Random(seed)
        roster, users, rooms = fuzz_roster(rng, 1025, 700, 5000)
        slots = pick_lookers(rng, 1025)
        out.append([digest(roster.who_many(slots, now=5000, date=DATE)), digest(roster.who_many(slots, now=5000, date=DATE))])
        roster.close()
    return {"same_on_a_second_call": out[0][0] == out[0][1], "same_on_a_second_roster": out[0] == out[1]}


def nothing_else_moved_part() -> dict:
    cap = 300
    rooms = fuzz_rooms()

    def build():
        r = device.Roster(cap, review_rooms=2, look_rooms=len(rooms))
        r.update(list(range(cap)), room=[j % 2 for j in range(cap)], colour=[j % 3 == 0 for j in range(cap)],
                 name=[b"U%d" % j for j in range(cap)], level=2)
        r.update([0, 1], name=[b"Alice", b"Bobby"])
        set_rooms(r, rooms)
        return r

    fresh, asked = build(), build()
    out = {"capacity": cap, "look_rooms": len(rooms), "lookers": 3, "fresh": other_calls(fresh), "before_who": other_calls(asked)}
    h = {}
    call = lambda: asked.who_many([0, 1, 2], now=77, date=DATE).timing["h2d_bytes"]
    h["first"] = call()
    h["clean"] = [call() for _ in range(2)]
    asked.update(7, last_login=5)
    h["after_last_login_update"] = call()
    asked.update(7, desc=b"changed")
    h["after_desc_update"] = call()
    h["clean_again"] = call()
    out["who_h2d"] = h

    def look(r):
        lk = r.look_many([0, 1])
        return [lk.output(0).hex(), lk.timing["h2d_bytes"]]

    out["look_after_who"], out["look_fresh"] = look(asked), look(fresh)
    out["after_who"] = other_calls(asked)                               # and the other calls still answer alike
    out["fresh_again"] = other_calls(fresh)
    fresh.close()
    asked.close()
    return out


def golden_part() -> dict:
    rooms = default_rooms()
    roster = device.Roster(8, look_rooms=len(rooms))
    set_rooms(roster, rooms)
    vs_model = []

    def answer(users, rooms_, slot, now, date):
        for u in users.values():
            seat(roster, u)
        got = roster.who_many([slot], now=now, date=date)
        if got.chunks(0) != model_chunks(users, rooms_, slot, now, date):
            vs_model.append(slot)
        return got.output(0)

    res = replay_whos(answer)
    roster.close()
    return {"compared": res["compared"], "mismatches": res["mismatches"][:2], "n_bad_vs_model": len(vs_model), "kinds": res["kinds"]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261)
    args = ap.parse_args()
    if device.device_count() < 1:
        print("no GPU visible", file=sys.stderr)
        return 3
    res = {"golden": golden_part(), "fuzz": fuzz_part(args.seed), "worst": worst_part(),
           "determinism": determinism_part(args.seed + 2), "moved": nothing_else_moved_part()}
    print("DEVICE_WHO " + json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
