"""The device work of tests/test_device_tell.py, in a short-lived child process of its own, and the CPU model the host
tier of that module shares with it.

As tests/device_speak_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_TELL {...}``).  ``private`` is the Python model of ``tell()``, ``pemote()`` and
``private_blocked()`` with ``get_user`` as the sequential two-pass loop of nuts333.c:2362-2379, built from the
reference's format strings and from ``np_wordfind`` / ``np_remove_first`` of the restatement.  ``lookup_rule`` is the
lookup of nuts_roster_tell in numpy: one row per slot, names packed in twelve bytes, the thirteen offsets, two minima.
``replay_private`` runs a recorded session of tests/golden: every line goes through ``dispatch`` of
tests/device_input_child.py, the commands that change what a later tell reads are applied, and every step that
dispatches to tell or pemote, and every ``.revtell``, is answered and compared with what each client received.

    python tests/device_tell_child.py [--seed S]
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

from device_input_child import COMMAND, dispatch, fuzz_read  # noqa: E402
from device_speak_child import SAY, fuzz_inpstr  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402

TELL, PEMOTE = device.COM_TELL, device.COM_PEMOTE
COMS = (TELL, PEMOTE)
TOLD, MUZZLED, NOTHING, NOBODY, SELF, AFK, IGNALL, IGNTELL, OFFSITE = (
    device.TOLD, device.MUZZLED, device.NOTHING, device.NOBODY, device.SELF, device.AFK, device.IGNALL, device.IGNTELL,
    device.OFFSITE)
OUTCOMES = (TOLD, MUZZLED, NOTHING, NOBODY, SELF, AFK, IGNALL, IGNTELL, OFFSITE)
MUZZLED_NOTICE = {TELL: b"You are muzzled, you cannot tell anyone anything.\n",     # nuts333.c:4134
                  PEMOTE: b"You are muzzled, you cannot emote.\n"}                  # nuts333.c:4236
WHAT_NOTICE = {TELL: b"Tell who what?\n", PEMOTE: b"Private emote what?\n"}         # nuts333.c:4138, 4240
SELF_NOTICE = {TELL: b"Talking to yourself is the first sign of madness.\n",        # nuts333.c:4146
               PEMOTE: b"Emoting to yourself is the second sign of madness.\n"}     # nuts333.c:4245
NOBODY_NOTICE = b"There is no one of that name logged on.\n"                        # nuts333.h notloggedon
IGNORED_WHAT = {TELL: b"tells", PEMOTE: b"private emotes"}
WIZ = 2
WORD_LEN = 40
REVTELL_HEADER, REVTELL_FOOTER = b"\n~BB~FG*** Your revtell buffer ***\n\n", b"\n~BB~FG*** End ***\n\n"   # c:7707, 7713
REVTELL_EMPTY = b"Revtell buffer is empty.\n"
GOLDEN = ("errors", "filters", "afk_bcast", "speech_colour_off", "speech_colour_mixed", "swearing", "markup", "review",
          "framing")
#: the steps of each session that dispatch to tell or pemote, and its .revtell steps
GOLDEN_PRIVATE_STEPS = {"errors": 7, "filters": 5, "afk_bcast": 3, "speech_colour_off": 6, "speech_colour_mixed": 4,
                        "swearing": 1, "markup": 1, "review": 10, "framing": 1}
#: and the comparisons they give: those steps x logged-in clients
GOLDEN_COMPARISONS = {"errors": 28, "filters": 20, "afk_bcast": 12, "speech_colour_off": 18, "speech_colour_mixed": 12,
                      "swearing": 2, "markup": 2, "review": 20, "framing": 2}


# ------------------------------------------------------------------ the model
def word_1(inpstr: bytes) -> bytes:
    """word[1] of the line whose inpstr this is: np_wordfind's first word of inpstr, cut at 39 bytes."""
    words = ctypes.create_string_buffer(10 * (WORD_LEN + 1))
    return words.raw[:WORD_LEN + 1].split(b"\0", 1)[0] if nuts_path.lib().np_wordfind(inpstr, words) else b""


def capitalised(word: bytes) -> bytes:
    """toupper() of the first byte in the C locale (get_user c:2366, pemote c:4243)."""
    return word[:1].upper() + word[1:] if word[:1].isalpha() and word[:1].isascii() else word


def get_user(users: dict, word: bytes):
    """nuts333.c:2362-2379 over the slots in ascending order: the exact pass, then the strstr pass; None: nobody."""
    name = capitalised(word)
    order = [users[j] for j in sorted(users) if not users[j]["login"] and users[j]["name"]]
    for u in order:
        if u["name"] == name:
            return u["slot"]
    for u in order:
        if name in u["name"]:
            return u["slot"]
    return None


def private(users: dict, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
    """What tell() / pemote() do for the speaker ``users[slot]``: the outcome, the slot get_user found (None: nobody,
    or not asked), the reply to the speaker and the line to the target (None: not told)."""
    u = users[slot]
    out = {"outcome": TOLD, "target": None, "reply": None, "line": None}
    if u["muzzled"]:
        return {**out, "outcome": MUZZLED, "reply": MUZZLED_NOTICE[com]}
    if word_count < 3:
        return {**out, "outcome": NOTHING, "reply": WHAT_NOTICE[com]}
    word = word_1(inpstr)
    if com == PEMOTE and capitalised(word) == u["name"]:                 # c:4243-4247, before get_user
        return {**out, "outcome": SELF, "reply": SELF_NOTICE[com]}
    found = get_user(users, word)
    if found is None:
        return {**out, "outcome": NOBODY, "reply": NOBODY_NOTICE}
    out["target"] = found
    if com == TELL and found == slot:                                   # c:4145
        return {**out, "outcome": SELF, "reply": SELF_NOTICE[com]}
    t = users[found]
    deaf = u["level"] < WIZ or t["level"] > u["level"]
    if t["afk"]:                                                        # private_blocked, c:4149-4172 / 4251-4273
        reply = (b"%s is AFK, message is: %s\n" % (t["name"], t["afk_mesg"]) if t["afk_mesg"]
                 else b"%s is AFK at the moment.\n" % t["name"])
        return {**out, "outcome": AFK, "reply": reply}
    if t["ignall"] and deaf:
        return {**out, "outcome": IGNALL, "reply": b"%s is ignoring everyone at the moment.\n" % t["name"]}
    if t["igntell"] and deaf:
        return {**out, "outcome": IGNTELL, "reply": b"%s is ignoring %s at the moment.\n" % (t["name"], IGNORED_WHAT[com])}
    if t["room"] is None:
        return {**out, "outcome": OFFSITE, "reply": b"%s is offsite and would not be able to reply to you.\n" % t["name"]}
    rest = nuts_path.lib().np_remove_first(inpstr)
    shown = u["name"] if u["vis"] else device.INVISNAME
    if com == TELL:
        verb = b"ask" if rest[-1:] == b"?" else b"tell"                 # c:4174
        return {**out, "reply": b"~OLYou %s %s:~RS %s\n" % (verb, t["name"], rest),
                "line": b"~OL%s %ss you:~RS %s\n" % (shown, verb, rest)}
    return {**out, "reply": b"~OL(To %s)~RS %s %s\n" % (t["name"], shown, rest),
            "line": b"~OL>>~RS %s %s\n" % (shown, rest)}


# ------------------------------------------------------------------ nuts_roster_tell's lookup, as the kernel does it
def lookup_rule(names: np.ndarray, nlen: np.ndarray, login: np.ndarray, words) -> np.ndarray:
    """get_user for a batch of words over one roster, as nuts_roster_tell does it: ``names`` is (cap, 12) bytes padded
    with zeros, one row per slot; a word longer than 12 bytes matches nobody; the word's first 12 bytes are packed as a
    name is, the first capitalised; a slot with the login flag or without a name is skipped; row j is an exact match
    if the lengths agree and the bytes are equal, a substring match if the word lies at one of the offsets 0 .. nlen -
    wlen; the answer is the minimum over the exact rows, else over the substring rows, else -1."""
    cap, nw = len(names), len(words)
    wlen = np.array([len(w) for w in words])
    packed = np.zeros((nw, 12), dtype=np.uint8)
    for r, w in enumerate(words):
        w = capitalised(w)[:12]
        packed[r, :len(w)] = np.frombuffer(w, dtype=np.uint8)
    wide = np.zeros((cap, 24), dtype=np.uint8)
    wide[:, :12] = names
    live = (~login & (nlen > 0))[None, :] & (wlen <= 12)[:, None]
    masked = np.arange(12)[None, None, :] >= wlen[:, None, None]         # bytes of the window the word does not cover
    exact = np.zeros((nw, cap), dtype=bool)
    sub = np.zeros((nw, cap), dtype=bool)
    for o in range(13):
        hit = ((wide[None, :, o:o + 12] == packed[:, None, :]) | masked).all(axis=2) & (o + wlen[:, None] <= nlen[None, :])
        if o == 0:
            exact = hit & (wlen[:, None] == nlen[None, :]) & live
        sub |= hit & live
    slots = np.arange(cap)[None, :]
    big = np.iinfo(np.int64).max
    best_exact = np.where(exact, slots, big).min(axis=1)
    best_sub = np.where(sub, slots, big).min(axis=1)
    return np.where(best_exact < big, best_exact, np.where(best_sub < big, best_sub, -1))


def packed_names(users: dict, cap: int):
    names, nlen, login = np.zeros((cap, 12), dtype=np.uint8), np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=bool)
    for j, u in users.items():
        if u["name"]:
            names[j, :len(u["name"])] = np.frombuffer(u["name"], dtype=np.uint8)
            nlen[j] = len(u["name"])
        login[j] = bool(u["login"])
    return names, nlen, login


# ------------------------------------------------------------------ the revtell rings
class TellRings:
    """A revtell ring per slot as the talker keeps them: np_record(ring, 5, ...) to store, .revtell to read."""
    LINES, SLOT = device.REVTELL_LINES, device.REVIEW_LEN + 2

    def __init__(self, slots: int):
        self.ring = [ctypes.create_string_buffer(self.LINES * self.SLOT) for _ in range(slots)]
        self.revline = [ctypes.c_int(0) for _ in range(slots)]

    def record(self, slot: int, text: bytes) -> None:
        nuts_path.lib().np_record(self.ring[slot], self.LINES, ctypes.byref(self.revline[slot]), text)

    def clear(self, slot: int) -> None:
        for i in range(self.LINES):
            self.ring[slot][i * self.SLOT] = b"\0"
        self.revline[slot].value = 0

    def lines(self, slot: int) -> list[bytes]:
        raw, rev = self.ring[slot].raw, self.revline[slot].value
        rows = [raw[s * self.SLOT:(s + 1) * self.SLOT].split(b"\0", 1)[0]
                for s in ((rev + i) % self.LINES for i in range(self.LINES))]
        return [line for line in rows if line]

    def chunks(self, slot: int, colour: int) -> list[bytes]:
        return [c for line in self.lines(slot) for c in nuts_path.chunks(line, colour)]


# ------------------------------------------------------------------ a roster and its model
FIELDS = ("room", "login", "ignall", "colour", "name", "vis", "muzzled", "level", "afk", "igntell", "afk_mesg")


def seat(roster: device.Roster, u: dict) -> None:
    """Slot u["slot"] of the roster in the state the model's user is in (a user without a name keeps none)."""
    fields = {f: u[f] for f in FIELDS if f != "name"}
    if u["name"]:
        fields["name"] = u["name"]
    roster.update(u["slot"], **fields)


def new_user(slot: int, **fields) -> dict:
    return {"slot": slot, "room": 0, "login": 0, "ignall": 0, "colour": 0, "name": None, "vis": 1, "muzzled": 0,
            "level": 1, "afk": 0, "igntell": 0, "afk_mesg": b"", "command_mode": 0, **fields}


SPECIAL_SLOTS = (0, 63, 64, 255, 256)


def private_roster(rng: random.Random, cap: int, revtell: bool = False, review_rooms: int = 0):
    """A roster of ``cap`` slots in a random state with names that share substrings, its model, the valid speakers, and
    the planted slots: 12-byte names at slots 0, 63, 64, 255, 256 and cap - 1, a substring match below an exact match,
    two substring matches, a matching slot that is logging in, one without a room, one without a name."""
    roster = device.Roster(cap, review_rooms=review_rooms, revtell=revtell)
    users = {}
    syll = (b"al", b"ice", b"bob", b"by", b"car", b"ol", b"dave", b"x", b"Zed", b"9", b"\xe9", b"an", b"na")
    for j in range(cap):
        name = None
        if rng.random() < 0.85:
            name = b"".join(rng.choice(syll) for _ in range(rng.randrange(1, 5)))[:rng.choice((12, 12, 5, 3))]
            name = name[:1].upper() + name[1:] if rng.random() < 0.8 else name
        users[j] = new_user(j, room=rng.choice((None, 0, 0, 0, 1, 2)), login=int(rng.random() < 0.1),
                            ignall=int(rng.random() < 0.2), colour=rng.randrange(2), name=name,
                            vis=int(rng.random() < 0.7), muzzled=int(rng.random() < 0.08),
                            level=rng.choice((0, 1, 1, 2, 3, 4)), afk=int(rng.random() < 0.12),
                            igntell=int(rng.random() < 0.2),
                            afk_mesg=rng.choice((b"", b"", b"back in five", b"m" * 60, b"~FRred~RS \xe9")))
    planted = sorted({s for s in SPECIAL_SLOTS + (cap - 1,) if 0 <= s < cap})
    for s in planted:
        users[s].update(name=b"Q%011d" % s, login=0, room=0, afk=0, ignall=0, igntell=0)
    if cap >= 63:
        users[10].update(name=b"Wilhelmina", login=0)                   # holds "Wil": below the exact match at 40
        users[40].update(name=b"Wil", login=0, room=0, afk=0, ignall=0, igntell=0)
        users[20].update(name=b"Gretchen1", login=0)                    # two hold "retch": the lower wins
        users[30].update(name=b"Gretchen2", login=0)
        users[5].update(name=b"Loginia", login=1)                       # skipped; slot 50 is found instead
        users[50].update(name=b"Loginia", login=0)
        users[7].update(name=b"Offsitia", login=0, room=None, afk=0, ignall=0, igntell=0)
        users[8].update(name=None)
        planted += [10, 40, 20, 30, 5, 50, 7]
    users[0].update(muzzled=0)
    for u in users.values():
        seat(roster, u)
    valid = [j for j, u in users.items() if u["room"] is not None and not u["login"] and u["name"]]
    return roster, users, valid, planted


FIRST_BYTES = (b"q", b"Q", b"9", b"\xe9", b"~", b"a", b"Z")


def fuzz_event(rng: random.Random, users: dict, valid, planted):
    """One (slot, com, inpstr, word_count): a word aimed at somebody (exact, a substring, a near miss, either case), at the
    speaker, or at nobody, of every length and first byte, with and without leading blanks, and a rest of every kind."""
    slot, com = rng.choice(valid), rng.choice(COMS)
    named = [j for j, u in users.items() if u["name"]]
    x = rng.random()
    if x < 0.6:
        nm = users[rng.choice(named if rng.random() < 0.5 else planted)]["name"] or b"Nobody"
        y = rng.random()
        if y < 0.45:
            w = nm
        elif y < 0.85:
            a = rng.randrange(len(nm))
            w = nm[a:rng.randrange(a + 1, len(nm) + 1)]
        else:
            w = rng.choice((nm + b"x", nm[:-1] + b"#", b"x" + nm))
        w = w[:1].lower() + w[1:] if rng.random() < 0.5 else w
    elif x < 0.72:
        nm = users[slot]["name"]
        w = rng.choice((nm, nm, nm[:1].lower() + nm[1:], nm[1:] or nm, nm[:-1] or nm))
    elif x < 0.86:
        w = rng.choice(FIRST_BYTES)[:1] + b"w" * (rng.choice((1, 12, 13, 39, 50)) - 1)
    else:
        w = rng.choice((b"", b"nobodyhere", b"9", b"\xe9va", b"al", b"a", b"x"))
    lead = rng.choice((b"", b"", b"", b" ", b"  ", b"\xe9 \x01"))
    y = rng.random()
    rest = (b"" if y < 0.1 else rng.choice((b" ", b" hello", b" are you there?", b"  ~FRred~RS text /~OL", b" ?", b"\xe9tail"))
            if y < 0.5 else b" " + fuzz_inpstr(rng))
    inpstr = (lead + w + rest)[:999].replace(b"\0", b"\x01")
    return slot, com, inpstr, rng.choice((3, 3, 3, 3, 3, 4, 9, 10, 2, 0))


def systematic_events(users: dict, valid, planted) -> list:
    """The edges the lookup can get wrong, whoever speaks: every planted slot by its exact name, in lower case, by a
    substring; exact above substring; two substrings; the skipped slots; oneself; an empty and a 999-byte inpstr."""
    who = valid[len(valid) // 2]
    out = []
    for s in planted:
        nm = users[s]["name"]
        for com in COMS:
            out += [(who, com, nm + b" by name", 4), (who, com, nm.lower() + b" lower?", 3), (who, com, b" " + nm[1:] + b" sub", 3),
                    (who, com, nm[2:7] + b" short sub", 4)]
    me = users[who]["name"]
    for com in COMS:
        out += [(who, com, w + b" hello?", 3) for w in (b"wil", b"Wil", b"retch", b"Gretchen", b"loginia", b"offsitia", me,
                                                         me[:1].lower() + me[1:], me[1:], me + b"x", b"w" * 50, b"w" * 39)]
        out += [(who, com, b"", 3), (who, com, b"", 0), (who, com, me, 3), (who, com, b"x" * 999, 3),
                (who, com, (me + b" " + b"y" * 999)[:999], 3), (who, com, (b"w" * 50 + b" " + b"?" * 999)[:999], 3)]
    return out


# ------------------------------------------------------------------ comparing a Private with the model
def private_differences(roster: device.Roster, users: dict, events, pv: device.Private, counts: dict) -> list:
    bad = []
    for k, (slot, com, inpstr, wc) in enumerate(events):
        m = private(users, slot, com, inpstr, wc)
        counts["outcome_by_com"][(m["outcome"], com)] = counts["outcome_by_com"].get((m["outcome"], com), 0) + 1
        if m["outcome"] == TOLD:
            counts["targets"].add(m["target"])
            counts["self_by_substring"] += m["target"] == slot
        counts["word_lengths"].add(len(word_1(inpstr)))
        where = {"event": k, "slot": slot, "com": com, "inpstr": inpstr[:50].decode("latin-1"), "len": len(inpstr), "wc": wc}
        target = -1 if m["target"] is None else m["target"]
        if int(pv.outcome[k]) != m["outcome"] or int(pv.target[k]) != target:
            bad.append({**where, "what": "outcome", "device": [int(pv.outcome[k]), int(pv.target[k])],
                        "model": [m["outcome"], target]})
            continue
        if pv.line(k) != (m["line"] or b"") or pv.reply_text(k) != m["reply"]:
            bad.append({**where, "what": "text", "device": [pv.line(k)[:80].decode("latin-1"),
                                                             pv.reply_text(k)[:80].decode("latin-1")]})
            continue
        for plan, text, what, who in ((pv.told, m["line"], "told", m["target"]), (pv.reply, m["reply"], "reply", slot)):
            for c in (0, 1):
                want = nuts_path.chunks(text, c) if text is not None else []
                if plan.chunks(k, c) != want or int(plan.variant_sizes[k, c]) != sum(map(len, want)):
                    bad.append({**where, "what": f"{what} chunks", "colour": c,
                                "device": [len(x) for x in plan.chunks(k, c)], "model": [len(x) for x in want]})
            want = np.zeros(roster.capacity, dtype=bool)
            if text is not None:
                want[who] = True
            if not np.array_equal(plan.admitted(k), want):
                bad.append({**where, "what": f"{what} admitted"})
    return bad


def new_counts() -> dict:
    return {"outcome_by_com": {}, "targets": set(), "word_lengths": set(), "self_by_substring": 0}


# ------------------------------------------------------------------ the golden sessions
def replay_private(name: str, answer, revtell_lines) -> dict:
    """Session ``name`` of tests/golden, every line as the read ``send + "\\n"``: accounts are seated in slots as they log
    in, all in room 0; what user_input() does for an AFK user, and .afk, .igntell, .ignall, .vis / .invis, .colour and
    .quit, are applied; every step that dispatches to tell or pemote goes through ``answer(roster, users, slot, data,
    d)``, which returns (reply chunks per colour, line chunks per colour or None, target), and every .revtell through
    ``revtell_lines(roster, slot)`` (chunks per colour); every logged-in client's bytes are compared with what the
    reference sent it."""
    lib = nuts_path.lib()
    doc = json.loads((REPO / "tests" / "golden" / f"{name}.json").read_text())
    accounts = {}
    for group in doc["accounts"]:
        for acc in (group if isinstance(group, list) else [group]):
            accounts[acc["name"]] = acc
    roster = device.Roster(8, review_rooms=1, revtell=True)
    seats, users = {}, {}
    res = {"private_steps": 0, "comparisons": 0, "mismatches": [], "outcomes": {}}

    def compare(step, got_of):
        for actor, slot in seats.items():
            if users[slot]["login"]:
                continue                                                # it has left
            got, want = got_of(slot), step["recv"].get(actor, "").encode("latin-1")
            res["comparisons"] += 1
            if got != want:
                res["mismatches"].append({"send": step["send"], "actor": actor, "got": got.decode("latin-1"),
                                          "want": want.decode("latin-1")})

    for step in doc["steps"]:
        if step["op"] == "login":
            acc, slot = accounts[step["name"]], len(seats)
            seats[step["actor"]] = slot
            users[slot] = new_user(slot, name=acc["name"].encode("latin-1"), muzzled=int(bool(acc["muzzled"])),
                                   command_mode=int(bool(acc["command_mode"])), level=int(acc["level"]),
                                   colour=int(bool(acc["colour"])))
        elif step["op"] == "line":
            data = step["send"].encode("latin-1") + b"\n"
            u = users[seats[step["actor"]]]
            d = dispatch(u, data)
            if u["afk"]:                                                # user_input, nuts333.c:211s
                if u["afk"] == 2:                                       # locked: the line is the password, or nothing
                    if "Session unlocked" in step["recv"].get(step["actor"], ""):
                        u.update(afk=0, afk_mesg=b"")
                    continue
                u.update(afk=0, afk_mesg=b"")
            if d["kind"] != COMMAND:
                continue
            what = lib.np_command_name(d["com"]).decode()
            inpstr = data[d["start"]:d["start"] + d["size"]]
            if what in ("vis", "invis"):
                u["vis"] = int(what == "vis")
            elif what in ("colour", "ignall", "igntell"):
                u[what] ^= 1
            elif what == "quit":
                u["login"] = 1                                          # get_user no longer finds it
            elif what == "afk":                                         # afk(), nuts333.c:7409-7454
                lock = d["word_count"] > 1 and word_1(inpstr) == b"lock"
                mesg = lib.np_remove_first(inpstr) if lock else inpstr
                if d["word_count"] > 1 and len(mesg) > device.AFK_MESG_LEN:
                    continue
                u.update(afk=2 if lock else 1, afk_mesg=mesg if d["word_count"] > 1 and mesg else u["afk_mesg"])
            elif what in ("tell", "pemote", "revtell"):
                for s in users.values():
                    seat(roster, {**s, "afk": int(bool(s["afk"]))})
                res["private_steps"] += 1
                if what == "revtell":
                    lines = revtell_lines(roster, u["slot"])
                    c = u["colour"]
                    mine = (nuts_path.transduce(REVTELL_HEADER, c) + b"".join(lines[c]) + nuts_path.transduce(REVTELL_FOOTER, c)
                            if lines[c] else nuts_path.transduce(REVTELL_EMPTY, c))
                    compare(step, lambda slot: mine if slot == u["slot"] else b"")
                    continue
                reply, line, target, outcome = answer(roster, users, u["slot"], data, d)
                res["outcomes"][str(outcome)] = res["outcomes"].get(str(outcome), 0) + 1
                compare(step, lambda slot: (b"".join(reply[users[slot]["colour"]]) if slot == u["slot"] else b"")
                        + (b"".join(line[users[slot]["colour"]]) if line is not None and slot == target else b""))
    roster.close()
    return res


def model_answers():
    """replay_private's two answering functions from the model alone, with the rings it records into."""
    rings = TellRings(8)

    def answer(roster, users, slot, data, d):
        m = private(users, slot, d["com"], data[d["start"]:d["start"] + d["size"]], d["word_count"])
        if m["line"] is not None:
            rings.record(m["target"], m["line"])
        both = lambda t: None if t is None else {c: nuts_path.chunks(t, c) for c in (0, 1)}
        return both(m["reply"]), both(m["line"]), m["target"], m["outcome"]

    return answer, lambda roster, slot: {c: rings.chunks(slot, c) for c in (0, 1)}


def device_answers(found: dict):
    """The same over input_many -> tell_many(record=True) and revtell_many; everything is checked against the model on
    the way (``found``)."""
    rings = TellRings(8)

    def answer(roster, users, slot, data, d):
        inp = roster.input_many([(slot, data)])
        com, inpstr, wc = int(inp.com[0]), inp.inpstr(0), int(inp.word_count[0])
        if int(inp.kind[0]) != COMMAND or com != d["com"]:
            found.setdefault("bad", []).append({"what": "input_many", "data": data.decode("latin-1")})
        pv = roster.tell_many([(slot, com, inpstr, wc)], record=True)
        found.setdefault("bad", []).extend(private_differences(roster, users, [(slot, com, inpstr, wc)], pv,
                                                               found.setdefault("counts", new_counts())))
        if pv.line(0):
            rings.record(int(pv.target[0]), pv.line(0))
        both = lambda plan, there: {c: plan.chunks(0, c) for c in (0, 1)} if there else None
        return both(pv.reply, True), both(pv.told, bool(pv.line(0))), int(pv.target[0]), int(pv.outcome[0])

    def revtell_lines(roster, slot):
        rv = roster.revtell_many([slot])
        if rv.lines(0) != rings.lines(slot) or any(rv.chunks(0, c) != rings.chunks(slot, c) for c in (0, 1)):
            found.setdefault("bad", []).append({"what": "revtell_many", "slot": slot})
        return {c: rv.chunks(0, c) for c in (0, 1)}

    return answer, revtell_lines


def golden_part() -> dict:
    out = {}
    for name in GOLDEN:
        found: dict = {}
        res = replay_private(name, *device_answers(found))
        res["n_bad_vs_model"] = len(found.get("bad", []))
        res["first_bad_vs_model"] = found.get("bad", [])[:3]
        res["mismatches"] = res["mismatches"][:3]
        out[name] = res
    return out


# ------------------------------------------------------------------ seeded events
CAPACITIES = (1, 63, 64, 65, 255, 256, 257, 1000)
EVENTS_PER_CALL = 300


def json_counts(counts: dict) -> dict:
    return {"outcome_by_com": {f"{o}/{c}": n for (o, c), n in sorted(counts["outcome_by_com"].items())},
            "targets": sorted(counts["targets"]), "word_lengths": sorted(counts["word_lengths"]),
            "self_by_substring": int(counts["self_by_substring"])}


def fuzz_part(seed: int) -> dict:
    rng = random.Random(seed)
    counts = new_counts()
    res = {"capacities": [], "calls": 0, "events": 0, "n_bad": 0, "first_bad": [], "longest_inpstr": 0, "copies": []}
    for cap in CAPACITIES:
        roster, users, valid, planted = private_roster(rng, cap)
        with roster:
            res["capacities"].append(cap)
            edges = systematic_events(users, valid, planted)
            for call in range(2):
                events = edges[call::2][:EVENTS_PER_CALL // 2]
                events += [fuzz_event(rng, users, valid, planted) for _ in range(EVENTS_PER_CALL - len(events))]
                pv = roster.tell_many(events)
                bad = private_differences(roster, users, events, pv, counts)
                res["n_bad"] += len(bad)
                res["first_bad"] += bad[:5 - len(res["first_bad"])]
                res["calls"] += 1
                res["events"] += len(events)
                res["longest_inpstr"] = max(res["longest_inpstr"], max(len(e[2]) for e in events))
                res["copies"].append([cap, len(events), pv.timing["h2d_bytes"], pv.timing["d2h_bytes"]])
    res.update(json_counts(counts))
    return res


def contract_part(seed: int) -> dict:
    """Every TOLD event's two plans equal plan_many of its own composed texts, chunks included; a void told plan is
    empty."""
    rng = random.Random(seed)
    res = {"checked": 0, "void": 0, "n_bad": 0, "first_bad": [], "coms": set()}
    roster, users, valid, planted = private_roster(rng, 300)
    with roster:
        events = systematic_events(users, valid, planted)[:120] + [fuzz_event(rng, users, valid, planted) for _ in range(180)]
        pv = roster.tell_many(events)
        told = [k for k in range(len(events)) if pv.outcome[k] == TOLD][:60]
        plans = roster.plan_many([(text, None, None, 0, events[k][1]) for k in told for text in (pv.line(k), pv.reply_text(k))])
        for i, k in enumerate(told):
            res["checked"] += 1
            res["coms"].add(events[k][1])
            for plan, at in ((pv.told, 2 * i), (pv.reply, 2 * i + 1)):
                same = all(plan.chunks(k, c) == plans.chunks(at, c) and plan.variant(k, c) == plans.variant(at, c)
                           for c in (0, 1))
                if not same:
                    res["n_bad"] += 1
                    res["first_bad"] += [{"event": k, "inpstr": events[k][2][:40].decode("latin-1")}][:5 - len(res["first_bad"])]
        for k in range(len(events)):
            if pv.outcome[k] != TOLD:
                res["void"] += 1
                if (pv.told.admitted(k).any() or pv.told.variant_sizes[k].any() or pv.told.write_counts[k].any()
                        or pv.line(k) != b"" or pv.told.chunks(k, 0) != [] or pv.told.chunks(k, 1) != []):
                    res["n_bad"] += 1
                    res["first_bad"] += [{"event": k, "what": "a void told plan is not empty"}][:5 - len(res["first_bad"])]
    res["coms"] = sorted(res["coms"])
    return res


def recording_run(seed: int) -> dict:
    """Rings against sequential np_record(..., 5, ...) over several calls: more than 5 and more than 64 tells to one
    target in one call, two targets interleaved, clear_revtell between calls, calls that do not record."""
    rng = random.Random(seed)
    cap = 130
    res = {"tell_calls": 0, "clears": 0, "reviews": 0, "recorded": 0, "lines_compared": 0, "most_to_one_target_in_one_call": 0,
           "n_bad": 0, "first_bad": [], "digest": []}
    roster, users, valid, planted = private_roster(rng, cap, revtell=True)
    rings = TellRings(cap)
    a, b = planted[1], planted[2]                                      # slots 63 and 64: never blocked

    def review():
        slots = sorted(set(valid[:20] + planted + [a, b]))
        rv = roster.revtell_many(slots + [a])                           # a duplicate at the end
        for q, slot in enumerate(slots + [a]):
            want = rings.lines(slot)
            res["lines_compared"] += len(want)
            if rv.lines(q) != want or any(rv.chunks(q, c) != rings.chunks(slot, c) for c in (0, 1)) \
                    or int(rv.line_counts[q]) != len(want):
                res["n_bad"] += 1
                res["first_bad"] += [{"slot": slot, "device": len(rv.lines(q)), "model": len(want)}][:5 - len(res["first_bad"])]
        res["digest"].append([rv.stored.tobytes().hex()[:40], int(rv.variant_sizes.sum()), rv.line_counts.tolist()])
        res["reviews"] += 1

    def tell(events, record=True):
        pv = roster.tell_many(events, record=record)
        per = {}
        for k, (slot, com, inpstr, wc) in enumerate(events):
            m = private(users, slot, com, inpstr, wc)
            if pv.line(k) != (m["line"] or b""):
                res["n_bad"] += 1
            if record and m["line"] is not None:
                rings.record(m["target"], m["line"])
                per[m["target"]] = per.get(m["target"], 0) + 1
                res["recorded"] += 1
        res["most_to_one_target_in_one_call"] = max([res["most_to_one_target_in_one_call"], *per.values()])
        res["tell_calls"] += 1

    na, nb = users[a]["name"], users[b]["name"]
    speakers = [j for j in valid if j not in (a, b) and not users[j]["muzzled"]]
    long_tail = b"~FRred~RS " + b"z" * 250                              # a line of 200 bytes or more is cut
    with roster:
        review()                                                        # every ring is empty
        tell([(speakers[0], TELL, na + b" one", 3)])
        tell([(rng.choice(speakers), rng.choice(COMS), na + b" seven %d" % i, 4) for i in range(7)])
        review()
        tell([(rng.choice(speakers), rng.choice(COMS), (na if i % 3 else nb) + b" interleaved %d?" % i, 3) for i in range(40)])
        tell([(speakers[1], TELL, na + b" not recorded", 4)], record=False)
        review()
        tell([(rng.choice(speakers), TELL, na + b" many %d " % i + (long_tail if i % 7 == 0 else b""), 4) for i in range(150)])
        review()
        roster.clear_revtell([a, valid[3]])
        rings.clear(a)
        rings.clear(valid[3])
        res["clears"] += 1
        tell([(speakers[2], PEMOTE, na + b" after the clear", 5), (speakers[2], PEMOTE, nb + b" waves", 3)])
        review()
        roster.clear_revtell(b)
        rings.clear(b)
        res["clears"] += 1
        review()                                                        # the clear travels with a review too
        for _ in range(4):
            events = [fuzz_event(rng, users, valid, planted) for _ in range(rng.choice((1, 9, 70, 200)))]
            tell(events, record=rng.random() < 0.8)
            if rng.random() < 0.5:
                slot = rng.choice(valid)
                roster.clear_revtell(slot)
                rings.clear(slot)
                res["clears"] += 1
        review()
    return res


def recording_part(seed: int) -> dict:
    first, second = recording_run(seed), recording_run(seed)
    first["same_on_a_second_run"] = first["digest"] == second["digest"] and first["n_bad"] == second["n_bad"]
    first["digest"] = len(first["digest"])
    return first


def nothing_else_moved_part() -> dict:
    """broadcast_many, plan_many (with and without record), review_many, speak_many and input_many give the same results
    and copy the same bytes on a fresh roster, after tell_many and revtell_many calls, and after updates of afk, igntell
    and afk_mesg alone; tell_many's copies are reported beside them."""
    out = {}
    rng = random.Random(23)
    roster, users, valid, planted = private_roster(rng, 300, revtell=True, review_rooms=3)
    calls = [(b"Uaaa says: line %d ~FRred~RS\n" % i, rng.choice((None, 0, 1)), rng.choice((None, 5)), 0, SAY)
             for i in range(20)]
    recorded = [(b"recorded %d\n" % i, i % 3, None, 0, SAY) for i in range(6)]
    speech = [(rng.choice(valid), rng.choice((3, 4, 6, 7)), fuzz_inpstr(rng), rng.randrange(11)) for _ in range(60)]
    reads = [(rng.choice(valid), fuzz_read(rng)) for _ in range(100)]
    tells = [fuzz_event(rng, users, valid, planted) for _ in range(100)]

    def snapshot():
        p, f = roster.plan_many(calls), roster.broadcast_many(calls)
        pr = roster.plan_many(recorded, record=True)
        s, i, v = roster.speak_many(speech, ban_swearing=True), roster.input_many(reads), roster.review_many([0, 1, 2])
        roster.clear_review([0, 1, 2])                                  # so that the next snapshot reviews the same
        return {"plan": [p.admitted_bits.tobytes().hex()[:64], [p.variant(k, c).hex() for k in range(3) for c in (0, 1)],
                         p.variant_sizes.tolist(), p.write_counts.tolist(), pr.variant_sizes.tolist()],
                "fanout": [int(f.admitted.sum()), int(f.out_offsets[-1]), int(f.write_offsets[-1]), f.arena[:2000].tobytes().hex()],
                "speak": [s.outcome.tolist(), s.text_sizes.tolist(), [s.line(k).hex() for k in range(10)],
                          s.room.variant_sizes.tolist(), int(s.room.admitted_bits.view(np.uint8).sum())],
                "input": [i.kind.tolist(), i.com.tolist(), i.speech.outcome.tolist(), i.speech.text_sizes.tolist()],
                "review": [v.line_counts.tolist(), v.variant_sizes.tolist(), [x.hex() for x in v.lines(0)]],
                # plan, fanout, plan(record=), speak, input, review: [h2d, d2h] each
                "copies": [[r.timing["h2d_bytes"], r.timing["d2h_bytes"]] for r in (p, f, pr, s, i, v)]}

    with roster:
        snapshot()                                   # every kind of call once: the allocations have their sizes
        out["fresh"] = snapshot()                    # no private speech call yet
        t0 = roster.tell_many(tells, record=True).timing
        roster.revtell_many(valid[:5])
        snapshot()                                   # the allocation grew: its first call uploads the table again, as ever
        out["after_telling"] = snapshot()
        ta = roster.tell_many(tells, record=True).timing
        roster.revtell_many(valid[:5])
        out["after_telling_twice"] = snapshot()
        dirty = [roster._dirty, roster._speech_dirty]
        roster.update(valid[0], afk=1 - users[valid[0]]["afk"], igntell=1, afk_mesg=b"gone fishing")
        out["private_update_left_dirty"] = dirty + [roster._dirty, roster._speech_dirty]
        out["after_private_update"] = snapshot()
        t1 = roster.tell_many(tells).timing                             # the speaker state and the AFK messages travel
        t2 = roster.tell_many(tells).timing
        roster.update(valid[0], afk_mesg=b"")
        t3 = roster.tell_many(tells).timing                             # the AFK messages alone
        out["after_telling_again"] = snapshot()
        out["tell_h2d"] = {"first": t0["h2d_bytes"], "clean": [ta["h2d_bytes"], t2["h2d_bytes"]], "after_private_update": t1["h2d_bytes"],
                           "after_afk_mesg_update": t3["h2d_bytes"]}
        out["tell_d2h"] = sorted({t["d2h_bytes"] for t in (t0, ta, t1, t2, t3)})
        out["capacity"] = roster.capacity
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1741)
    a = ap.parse_args()
    out = {"device_count": device.device_count()}
    if out["device_count"] < 1:
        print("device_tell_child: no GPU visible", file=sys.stderr)
        return 2
    out["golden"] = golden_part()
    out["fuzz"] = fuzz_part(a.seed)
    out["contract"] = contract_part(a.seed + 1)
    out["recording"] = recording_part(a.seed + 2)
    out["moved"] = nothing_else_moved_part()
    print("DEVICE_TELL " + json.dumps(out, default=str))
    return 0


if __name__ == "__main__":
    sys.exit(main())
