"""The device work of tests/test_device_input.py, in a short-lived child process of its own, and the CPU model the host
tier of that module shares with it.

As tests/device_speak_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_INPUT {...}``).  ``dispatch`` is the Python model of ``user_input()`` and the front part of
``exec_com()``: ``np_terminate``, ``np_wordfind``, ``np_remove_first``, ``np_command_lookup`` and ``np_command_level``
of the restatement and the reference's control flow between them, each step with its nuts333.c line.  ``answer_of``
joins it with ``model`` of tests/device_speak_child.py into what ``Roster.input_many`` returns for a read.
``replay_reads`` runs a recorded session of tests/golden through them, every line as the read ``send + "\\n"``.
``parse_rule`` is nuts_roster_parse in numpy, with the kernel's lane slices, its carry between lanes, the modulo 39 and
the two table entries per lane.

    python tests/device_input_child.py [--seed S]
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
from device_speak_child import (COMS, EMOTE, GOLDEN, SAY, SEMOTE, SHOUT, SWEAR_WORDS, WHAT_NOTICE,  # noqa: E402
                                admitted_by_predicate, fuzz_inpstr, model, random_roster)
from nuts333_amd import device, nuts_path  # noqa: E402

IAC, EMPTY, REPEAT, UNKNOWN, SPEECH, COMMAND = (device.IAC, device.EMPTY, device.REPEAT, device.UNKNOWN, device.SPEECH,
                                                device.COMMAND)
KINDS = (IAC, EMPTY, REPEAT, UNKNOWN, SPEECH, COMMAND)
UNKNOWN_NOTICE = b"Unknown command.\n"                                  # nuts333.c:3763, 3782
SHORTCUTS = {b">": b"tell", b"<": b"pemote", b"-": b"echo", b"!": b"shout"}      # nuts333.c:3765-3768
WORD_LEN = 40                                                           # nuts333.h:18


def command_table() -> list[tuple[bytes, int]]:
    """(name, minimum level) of every command, in enum np_com's order, from the restatement."""
    lib = nuts_path.lib()
    return [(lib.np_command_name(c), lib.np_command_level(c)) for c in range(lib.np_command_count())]


# ------------------------------------------------------------------ the model
def dispatch(speaker: dict, data: bytes) -> dict:
    """What user_input() and exec_com() make of one read of ``speaker`` (command_mode, level) before a command function
    runs: kind, com (-1: none), word_count, the line's length, where inpstr starts in ``data`` and its length (-1:
    none), and whether a say is forced to "Say what?"."""
    lib = nuts_path.lib()
    out = {"kind": IAC, "com": -1, "word_count": 0, "line_size": 0, "start": 0, "size": -1, "forced": False}
    if data[0] == 255:                                                  # nuts333.c:150s: a telnet IAC reply
        return out
    buf = ctypes.create_string_buffer(data, len(data) + 1)
    n = lib.np_terminate(buf)                                           # nuts333.c:172 -> 403-411
    line = buf.raw[:n]
    words = ctypes.create_string_buffer(10 * (WORD_LEN + 1))
    wc = lib.np_wordfind(line, words)                                   # nuts333.c:197 -> 417-432
    out.update(word_count=wc, line_size=n)
    if line == b".":                                                    # nuts333.c:185: the caller's inpstr_old
        return {**out, "kind": REPEAT}
    if wc == 0:                                                         # nuts333.c:207-211
        return {**out, "kind": EMPTY}
    if not speaker["command_mode"] and line[:1] not in (b".", b";", b"!", b"<", b">", b"-", b"#"):     # c:213-214
        return {**out, "kind": SPEECH, "com": SAY, "size": n}
    word0 = words.raw[:WORD_LEN + 1].split(b"\0", 1)[0]
    dotted = word0[:1] == b"."
    comword = word0[1:] if dotted else word0                            # nuts333.c:3761-3762
    if not comword:                                                     # nuts333.c:3763
        return {**out, "kind": UNKNOWN}
    if word0 in SHORTCUTS:                                              # nuts333.c:3765-3768: comword is word[0] here
        comword = SHORTCUTS[word0]
    start = 0
    if line[:1] == b";":                                                # nuts333.c:3769
        comword = b"emote"
    elif line[:1] == b"#":                                              # nuts333.c:3770
        comword = b"semote"
    else:
        start = n - len(lib.np_remove_first(line))                      # nuts333.c:3771 -> 2350-2358
    com = lib.np_command_lookup(comword)                                # nuts333.c:3776-3781
    if com == -1 or lib.np_command_level(com) > speaker["level"]:       # nuts333.c:3782
        return {**out, "kind": UNKNOWN}
    out.update(com=com, start=start, size=n - start, kind=SPEECH if com in COMS else COMMAND)
    out["forced"] = com == SAY and wc < 2                               # nuts333.c:3826-3829
    return out


def answer_of(speaker: dict, data: bytes, ban_swearing: bool) -> tuple[dict, dict]:
    """dispatch() of the read, and what is written for it as model() states it."""
    d = dispatch(speaker, data)
    void = {"outcome": device.NOT_SPEECH, "reply": None, "line": None, "rm": None, "sender": None, "recorded": False}
    if d["kind"] == UNKNOWN:
        return d, {**void, "reply": UNKNOWN_NOTICE}
    if d["kind"] != SPEECH:
        return d, void
    if d["forced"]:
        return d, {**void, "outcome": device.NOTHING, "reply": WHAT_NOTICE[SAY]}
    return d, model(speaker, d["com"], data[d["start"]:d["start"] + d["size"]], d["word_count"], ban_swearing)


# ------------------------------------------------------------------ nuts_roster_parse, as the kernel does it
def _first_from(bits: np.ndarray, start: np.ndarray, none: np.ndarray) -> np.ndarray:
    """first_from of fanout.hip over (B, 64, 16) mask bits: a ballot over "my slice has a bit at or after start" gives
    the lane, that lane's lowest such bit the index."""
    b = np.arange(len(bits))
    at = 16 * np.arange(64)[None, :, None] + np.arange(16)[None, None, :]
    m = bits & (at >= start[:, None, None])
    ballot = m.any(axis=2)
    lane = ballot.argmax(axis=1)
    return np.where(ballot.any(axis=1), 16 * lane + m[b, lane].argmax(axis=1), none)


def _packed_names():
    """The command table as fanout.hip packs it: bytes 0 .. 7 of a name in one word, 8 and 9 in another, levels."""
    table = command_table()
    lo = np.zeros(128, dtype=np.uint64)
    hi = np.zeros(128, dtype=np.uint64)
    level = np.zeros(128, dtype=np.int64)
    for c, (name, lv) in enumerate(table):
        assert len(name) <= 10
        lo[c] = int.from_bytes(name[:8], "little")
        hi[c] = int.from_bytes(name[8:], "little")
        level[c] = lv
    return lo, hi, level, len(table)


def parse_rule(datas, command_mode, level) -> dict:
    """nuts_roster_parse over a batch of reads: per read kind, com, word_count, line_size, start, size and forced, as
    arrays.  Lane l of 64 owns bytes 16l .. 16l+15; the distance a slice's first byte inherits from its run comes from
    the nearest lane below that is not all word bytes; a word starts where the distance is a multiple of 39; lane l
    tests table entries l and l + 64."""
    nb = len(datas)
    b = np.arange(nb)
    raw = np.zeros((nb, 1024), dtype=np.uint8)
    lens = np.array([len(d) for d in datas])
    for r, d in enumerate(datas):
        raw[r, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    command_mode, level = np.asarray(command_mode, dtype=bool), np.asarray(level)
    at = np.arange(1024)
    signed = np.where(at[None, :] < lens[:, None], raw.view(np.int8).astype(np.int64), 0).reshape(nb, 64, 16)
    ends, wordb = signed < 32, signed > 32
    n = _first_from(ends, np.zeros(nb, dtype=np.int64), lens)
    wordb &= at.reshape(1, 64, 16) < n[:, None, None]

    # the carry: the nearest lane below that ends a run, its trailing word bytes, and 16 per full lane between
    full = wordb.all(axis=2)
    lanes = np.arange(64)
    below = np.where(~full, lanes[None, :], -1)
    prev = np.concatenate([np.full((nb, 1), -1), np.maximum.accumulate(below, axis=1)[:, :-1]], axis=1)
    tail = np.cumprod(wordb[:, :, ::-1], axis=2).sum(axis=2)            # trailing word bytes of a slice
    carry = np.where(prev < 0, 16 * lanes[None, :], 16 * (lanes[None, :] - 1 - prev) + tail[b[:, None], np.maximum(prev, 0)])
    dist = carry % 39
    total = np.zeros(nb, dtype=np.int64)
    for x in range(16):
        w = wordb[:, :, x]
        total += (w & (dist == 0)).sum(axis=1)
        dist = np.where(w, np.where(dist == 38, 0, dist + 1), 0)
    wc = np.where(total >= 10, 9, total)

    b0 = raw[:, 0]
    w0 = _first_from(wordb, np.zeros(nb, dtype=np.int64), n)
    w0_end = _first_from(~wordb, w0, n)
    rest = _first_from(wordb, w0_end, n)
    wlen = np.minimum(w0_end - w0, 39)
    first = raw[b, np.minimum(w0, 1023)]
    cw = w0 + (first == ord("."))
    cwlen = w0 + wlen - cw

    # the lookup: comword packed as the names are, two entries per lane, the lowest set bit of the two ballots
    lo, hi = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
    for i in range(10):
        c = np.where(i < cwlen, raw[b, np.minimum(cw + i, 1023)], 0).astype(np.uint64)
        if i < 8:
            lo |= c << np.uint64(8 * i)
        else:
            hi |= c << np.uint64(8 * (i - 8))
    mlo = np.where(cwlen >= 8, np.uint64(2**64 - 1), (np.uint64(1) << (8 * np.clip(cwlen, 0, 7)).astype(np.uint64)) - np.uint64(1))
    mhi = np.where(cwlen <= 8, np.uint64(0), (np.uint64(1) << (8 * np.clip(cwlen - 8, 0, 2)).astype(np.uint64)) - np.uint64(1))
    tlo, thi, tlevel, ncom = _packed_names()
    looked = np.full(nb, -1)
    for half in (1, 0):                                                 # entries l + 64, then l: the lower half wins
        e = half * 64 + lanes
        hit = ((tlo[e][None, :] & mlo[:, None]) == lo[:, None]) & ((thi[e][None, :] & mhi[:, None]) == hi[:, None])
        hit &= (e < ncom)[None, :]
        looked = np.where(hit.any(axis=1), half * 64 + hit.argmax(axis=1), looked)
    looked = np.where(cwlen <= 10, looked, -1)

    lead = np.isin(b0, list(b".;!<>-#"))
    direct = ~command_mode & ~lead
    com = looked
    short = (wlen == 1) & np.isin(first, list(b"><-!"))
    for ch, c in ((b">", 5), (b"<", 8), (b"-", 9), (b"!", 4)):
        com = np.where(short & (first == ch[0]), c, com)
    com = np.where(b0 == ord(";"), EMOTE, np.where(b0 == ord("#"), SEMOTE, com))
    start = np.where((b0 == ord(";")) | (b0 == ord("#")), 0, rest)
    com = np.where(cwlen > 0, com, -1)
    com = np.where((com >= 0) & (tlevel[np.maximum(com, 0)] > level), -1, com)
    speech = np.isin(com, COMS)
    kind = np.where(com < 0, UNKNOWN, np.where(speech, SPEECH, COMMAND))
    forced = (com == SAY) & (wc < 2)
    size = np.where(com < 0, -1, n - start)
    # the early outcomes, last first
    kind = np.where(direct, SPEECH, kind)
    com = np.where(direct, SAY, com)
    start = np.where(direct | (com < 0), 0, start)
    size = np.where(direct, n, size)
    forced &= ~direct
    for cond, k in ((total == 0, EMPTY), ((n == 1) & (b0 == ord(".")), REPEAT), (b0 == 255, IAC)):
        kind = np.where(cond, k, kind)
        com, start, size, forced = np.where(cond, -1, com), np.where(cond, 0, start), np.where(cond, -1, size), forced & ~cond
    return {"kind": kind, "com": com, "word_count": wc, "line_size": n, "start": start, "size": size, "forced": forced}


# ------------------------------------------------------------------ seeded reads
TERMINATORS = (b"\n", b"\n", b"\r\n", b"\0", b"\x80", b"\xff", b"\x1f", b"\x9b", b"\n\0trailing\n", b"\r\0", b"\n more\x1f")
NAMES = None


def fuzz_read(rng: random.Random) -> bytes:
    """One read: a body of every kind the dispatcher tells apart, then a terminator (and sometimes bytes after it)."""
    global NAMES
    if NAMES is None:
        NAMES = [name for name, _ in command_table()]
    words = lambda k: b" ".join(rng.choice((b"hello", b"there", b"a", b"bobby", b"x" * 17, b"~FRred", b"?", b"ok!"))
                                for _ in range(k))
    run = lambda: b"w" * rng.choice((38, 39, 40, 77, 78, 79, 390, rng.randrange(1, 120)))
    x = rng.random()
    if x < 0.05:
        body = b"\xff" + bytes(rng.randrange(256) for _ in range(rng.randrange(0, 12)))
    elif x < 0.10:
        body = rng.choice((b"", b" ", b"   ", b" " * rng.randrange(1, 999)))
    elif x < 0.15:
        body = rng.choice((b".", b".", b".", b". ", b" .", b"..", b". x"))
    elif x < 0.40:                                                      # a command, a prefix of one, a near miss
        name = rng.choice(NAMES)
        name = name[:rng.randrange(1, len(name) + 1)] if rng.random() < 0.6 else name
        if rng.random() < 0.15:
            name = rng.choice((name + b"x", name[:-1] + b"Q", name.upper(), name + b"." , b"x" + name))
        body = rng.choice((b"", b"", b".", b".", b".", b" .", b"  ", b" ")) + name
        body += rng.choice((b"", b" ", b"  ")) + (fuzz_inpstr(rng)[:200] if rng.random() < 0.6 else words(rng.randrange(0, 4)))
    elif x < 0.55:                                                      # the shortcuts and what looks like them
        lead = rng.choice((b";", b"#", b"!", b"<", b">", b"-", b";", b"#", b"!x", b".!", b" ;x", b"..", b".;", b">x", b" >",
                           b" !", b"-x", b".#", b" #", b"<<"))
        body = lead + rng.choice((b"", b" ", b"")) + (fuzz_inpstr(rng)[:300] if rng.random() < 0.6 else words(rng.randrange(0, 4)))
    elif x < 0.64:                                                      # a speech command through exec_com, every outcome
        lead = rng.choice((b".shout", b".shout", b"!", b".sh", b".say", b".s", b"say", b".emote", b".semote", b";", b"#"))
        y = rng.random()
        if y < 0.2:                                                     # nothing to say: "Say what?" and its like
            arg = rng.choice((b"", b" ", b"  "))
        elif y < 0.6:                                                   # a swear word, any case, between other words
            w = bytes(rng.choice((ch, ch ^ 32)) for ch in rng.choice(SWEAR_WORDS))
            arg = b" " + words(rng.randrange(0, 3)) + rng.choice((b" ", b"x", b"")) + w + rng.choice((b"", b"!", b" ok"))
        else:
            arg = b" " + words(rng.randrange(1, 6))
        body = lead + arg
    elif x < 0.75:                                                      # a plain line: a say, or a command in command mode
        body = rng.choice((b"", b"", b" ", b"   ")) + fuzz_inpstr(rng)
    elif x < 0.90:                                                      # long runs, and totals around ten words
        body = rng.choice((b"", b" ", b".")) + b" ".join(run() if rng.random() < 0.5 else b"w" for _ in range(rng.randrange(1, 14)))
    else:
        body = bytes(rng.randrange(256) for _ in range(rng.choice((1, 5, 40, rng.randrange(1, 999)))))
    term = rng.choice(TERMINATORS)
    return body[:1000 - len(term)] + term


def systematic_reads() -> list[bytes]:
    """The edges: every command name and every proper prefix of one in every position, runs at the word length's
    multiples, totals of nine, ten and more words, terminators at the first and last index and around every slice
    boundary, bytes of 0x80 and above and NUL inside the read."""
    out = []
    for name, _ in command_table():
        for cut in range(1, len(name) + 1):
            for form in (b".%s\n", b"%s\n", b".%s some words here\n", b" .%s  x\n", b"%s two\r\n", b".%sx\n"):
                out.append(form % name[:cut])
    for length in (38, 39, 40, 77, 78, 79, 390):
        for lead in (b"", b" ", b".", b"x "):
            out += [lead + b"r" * length + b"\n", lead + b"r" * length + b" tail\n", lead + b"r" * length + b" " + b"q" * length + b"\x80"]
    for total in (8, 9, 10, 11, 12, 25):
        out += [b" ".join([b"w"] * total) + b"\n", b"." + b" ".join([b"w"] * total) + b"\n",
                b"w" * 39 * (total - 1) + b" w\n" if 39 * (total - 1) + 3 <= 1000 else b"w" * 997 + b" w\n"]
    for idx in [0, 999] + [16 * s + d for s in range(1, 63) for d in (-1, 0, 1) if 16 * s + d < 1000]:
        out += [b"x" * idx + b"\n", b"x" * idx + b"\x80" + b"y" * min(3, 999 - idx - 1) + (b"\n" if idx < 999 else b""),
                (b".shout " + b"x" * 1000)[:idx] + b"\0"]
    out += [b"ab\0cd\n", b"a\x80b\n", b"a\xe9 b\n", b"\x80\n", b"\0", b"\xff", b"\xff\xfb\x01", b"\xfe\n", b" \xff\n", b".\n", b".\r\n",
            b". \n", b" .\n", b"..\n", b"!x\n", b".!\n", b" ;x\n", b";\n", b"#\n", b"; x\n", b"!\n", b"! \n", b"! x y\n", b">\n",
            b"> bobby hi\n", b"< bobby waves\n", b"- echo this\n", b" - echo\n", b"say\n", b".say\n", b".say hi\n", b"s\n", b".s x\n"]
    return [r for r in out if 1 <= len(r) <= 1000 and not 32 <= r[-1] < 128]


# ------------------------------------------------------------------ the golden sessions
#: the commands of the recorded sessions that change what a later speech step reads: com -> what the replay toggles
STATE_COMMANDS = {"colour": "colour", "ignall": "ignall", "ignshout": "ignshout", "vis": "vis", "invis": "vis"}


def replay_reads(name: str, answer) -> dict:
    """tests/device_speak_child.replay with dispatch() in classify()'s place: every line step's read is ``send + "\\n"``,
    the levels come from the accounts, .colour / .ignall / .ignshout / .vis / .invis are applied by the ``com`` the
    model returns, and every SPEECH read goes through ``answer(roster, speakers, slot, data, ban)``, which returns
    (reply chunks per colour or None, line chunks per colour or None, admitted bools)."""
    lib = nuts_path.lib()
    doc = json.loads((REPO / "tests" / "golden" / f"{name}.json").read_text())
    ban = bool(doc.get("config", {}).get("ban_swearing", False))
    accounts = {}
    for group in doc["accounts"]:
        for acc in (group if isinstance(group, list) else [group]):
            accounts[acc["name"]] = acc
    roster = device.Roster(8, review_rooms=1)
    seats, speakers = {}, {}
    res = {"comparisons": 0, "speech_steps": 0, "mismatches": [], "kinds": {}}
    for step in doc["steps"]:
        if step["op"] == "login":
            acc, slot = accounts[step["name"]], len(seats)
            seats[step["actor"]] = slot
            speakers[slot] = {"slot": slot, "room": 0, "name": acc["name"].encode("latin-1"), "vis": 1,
                              "muzzled": int(bool(acc["muzzled"])), "command_mode": int(bool(acc["command_mode"])),
                              "level": int(acc["level"]), "colour": int(bool(acc["colour"])), "ignall": 0, "ignshout": 0}
        elif step["op"] == "line":
            data = step["send"].encode("latin-1") + b"\n"
            sp = speakers[seats[step["actor"]]]
            d = dispatch(sp, data)
            res["kinds"][str(d["kind"])] = res["kinds"].get(str(d["kind"]), 0) + 1
            if d["kind"] == COMMAND:
                what = lib.np_command_name(d["com"]).decode()
                if what in ("vis", "invis"):
                    sp["vis"] = int(what == "vis")
                elif what in STATE_COMMANDS:
                    sp[what] ^= 1
            if d["kind"] != SPEECH:
                continue
            for s in speakers.values():
                roster.update(s["slot"], room=s["room"], colour=s["colour"], ignall=s["ignall"], ignshout=s["ignshout"],
                              name=s["name"], vis=s["vis"], muzzled=s["muzzled"], command_mode=s["command_mode"],
                              level=s["level"])
            reply, line, admitted = answer(roster, speakers, sp["slot"], data, ban)
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


def model_answer(roster, speakers, slot, data, ban):
    d, m = answer_of(speakers[slot], data, ban)
    both = lambda t: None if t is None else {c: nuts_path.chunks(t, c) for c in (0, 1)}
    admitted = (admitted_by_predicate(roster, m["rm"], m["sender"], d["com"]) if m["line"] is not None
                else np.zeros(roster.capacity, dtype=bool))
    return both(m["reply"]), both(m["line"]), admitted


# ------------------------------------------------------------------ comparing an Input with the model
def input_differences(roster: device.Roster, speakers: dict, reads, ban: bool, inp: device.Input, counts: dict,
                      check_admits: bool = True) -> list:
    """What of an Input differs from the model: kind, com, word_count, the line and inpstr ranges, and of its Speech
    the outcome, both texts, both plans' chunks with both colours and who is admitted."""
    bad = []
    sp = inp.speech
    for k, (slot, data) in enumerate(reads):
        d, m = answer_of(speakers[slot], data, ban)
        counts["kinds"][d["kind"]] = counts["kinds"].get(d["kind"], 0) + 1
        if d["kind"] == SPEECH:
            key = (m["outcome"], d["com"])
            counts["speech"][key] = counts["speech"].get(key, 0) + 1
            counts["forced"] += d["forced"]
        where = {"read": k, "slot": slot, "data": data[:40].decode("latin-1"), "len": len(data), "model": d}
        got = {"kind": int(inp.kind[k]), "com": int(inp.com[k]), "word_count": int(inp.word_count[k]),
               "line_size": int(inp.line_sizes[k]), "start": int(inp.inpstr_starts[k]), "size": int(inp.inpstr_sizes[k])}
        if got != {f: int(d[f]) for f in got}:
            bad.append({**where, "what": "parse", "device": got})
            continue
        if inp.inpstr(k) != (data[d["start"]:d["start"] + d["size"]] if d["size"] >= 0 else b"") or inp.line(k) != data[:d["line_size"]]:
            bad.append({**where, "what": "accessors"})
        if int(sp.outcome[k]) != m["outcome"]:
            bad.append({**where, "what": "outcome", "device": int(sp.outcome[k]), "model_outcome": m["outcome"]})
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
                                "device": [len(x) for x in plan.chunks(k, c)], "want": [len(x) for x in want]})
        want = np.zeros(roster.capacity, dtype=bool)
        if m["reply"] is not None:
            want[slot] = True
        if not np.array_equal(sp.reply.admitted(k), want):
            bad.append({**where, "what": "reply admitted"})
        if m["line"] is None:
            if sp.room.admitted(k).any():
                bad.append({**where, "what": "a line that was not spoken admits someone"})
        elif check_admits:
            want = admitted_by_predicate(roster, m["rm"], m["sender"], d["com"])
            if not np.array_equal(sp.room.admitted(k), want):
                bad.append({**where, "what": "room admitted", "device": int(sp.room.admitted(k).sum()),
                            "want": int(want.sum())})
    return bad


def new_counts() -> dict:
    return {"kinds": {}, "speech": {}, "forced": 0}


def device_answer(found: dict):
    """replay_reads()'s answering function over input_many; the whole Input is checked against the model on the way."""
    def answer(roster, speakers, slot, data, ban):
        inp = roster.input_many([(slot, data)], ban_swearing=ban)
        found.setdefault("bad", []).extend(
            input_differences(roster, speakers, [(slot, data)], ban, inp, found.setdefault("counts", new_counts())))
        sp = inp.speech
        both = lambda plan, there: {c: plan.chunks(0, c) for c in (0, 1)} if there else None
        return both(sp.reply, bool(sp.reply_text(0))), both(sp.room, bool(sp.line(0))), sp.room.admitted(0)
    return answer


def levelled_roster(rng: random.Random, cap: int, review_rooms: int = 0):
    """random_roster of tests/device_speak_child.py with a level per slot."""
    roster, speakers, valid = random_roster(rng, cap, review_rooms=review_rooms)
    for j, s in speakers.items():
        s["level"] = rng.choice((0, 1, 1, 1, 2, 3, 4))
        roster.update(j, level=s["level"])
    return roster, speakers, valid


CAPACITIES = (1, 63, 64, 65, 300, 1000)
READS_PER_CALL = 300


def json_counts(counts: dict) -> dict:
    return {"kinds": {str(k): n for k, n in sorted(counts["kinds"].items())},
            "outcome_by_com": {f"{o}/{c}": n for (o, c), n in sorted(counts["speech"].items())},
            "forced": int(counts["forced"])}


def fuzz_part(seed: int) -> dict:
    rng = random.Random(seed)
    counts = new_counts()
    edges = systematic_reads()
    res = {"capacities": [], "calls": 0, "reads": 0, "n_bad": 0, "first_bad": [], "longest_read": 0, "copies": []}
    for cap in CAPACITIES:
        roster, speakers, valid = levelled_roster(rng, cap)
        with roster:
            res["capacities"].append(cap)
            for ban in (False, True):
                reads = [(rng.choice(valid), fuzz_read(rng)) for _ in range(READS_PER_CALL - 40)]
                reads += [(rng.choice(valid), rng.choice(edges)) for _ in range(40)]
                inp = roster.input_many(reads, ban_swearing=ban)
                bad = input_differences(roster, speakers, reads, ban, inp, counts)
                res["n_bad"] += len(bad)
                res["first_bad"] += bad[:5 - len(res["first_bad"])]
                res["calls"] += 1
                res["reads"] += len(reads)
                res["longest_read"] = max(res["longest_read"], max(len(r[1]) for r in reads))
                res["copies"].append([cap, len(reads), inp.timing["h2d_bytes"], inp.timing["d2h_bytes"]])
    res.update(json_counts(counts))
    return res


def _same_entry(a: device.Speech, k: int, b: device.Speech) -> bool:
    """Entry k of Speech a equals entry 0 of Speech b: outcome, texts and both plans."""
    if int(a.outcome[k]) != int(b.outcome[0]) or a.line(k) != b.line(0) or a.reply_text(k) != b.reply_text(0):
        return False
    for pa, pb in ((a.room, b.room), (a.reply, b.reply)):
        if not (np.array_equal(pa.admitted_bits[k], pb.admitted_bits[0]) and np.array_equal(pa.colour_bits, pb.colour_bits)
                and pa.capacity == pb.capacity and np.array_equal(pa.variant_sizes[k], pb.variant_sizes[0])
                and np.array_equal(pa.write_counts[k], pb.write_counts[0])
                and all(pa.variant(k, c) == pb.variant(0, c) and pa.chunks(k, c) == pb.chunks(0, c) for c in (0, 1))):
            return False
    return True


def contract_part(seed: int) -> dict:
    """input_many(reads).speech at k equals speak_many([(slot, com, inpstr(k), word_count)]) at 0 for every SPEECH read
    outside the forced case."""
    rng = random.Random(seed)
    res = {"checked": 0, "forced_skipped": 0, "n_bad": 0, "first_bad": [], "coms": set()}
    for cap in (65, 300):
        roster, speakers, valid = levelled_roster(rng, cap)
        with roster:
            reads = [(rng.choice(valid), fuzz_read(rng)) for _ in range(240)]
            reads += [(rng.choice(valid), data) for data in (b".say\n", b".s \r\n", b" .say\0")]     # forced, whoever says it
            for ban in (False, True):
                inp = roster.input_many(reads, ban_swearing=ban)
                picked = 0
                for k, (slot, data) in enumerate(reads):
                    if inp.kind[k] != SPEECH:
                        continue
                    if dispatch(speakers[slot], data)["forced"]:
                        res["forced_skipped"] += 1
                        continue
                    if picked >= 50:
                        continue
                    picked += 1
                    com = int(inp.com[k])
                    one = roster.speak_many([(slot, com, inp.inpstr(k), int(inp.word_count[k]))], ban_swearing=ban)
                    res["checked"] += 1
                    res["coms"].add(com)
                    if not _same_entry(inp.speech, k, one):
                        res["n_bad"] += 1
                        res["first_bad"] += [{"read": k, "com": com, "data": data[:40].decode("latin-1")}][:5 - len(res["first_bad"])]
    res["coms"] = sorted(res["coms"])
    return res


def recording_part(seed: int) -> dict:
    """Two rosters in the same state: one records through input_many(record=True), the other through
    speak_many(record=True) of the events the model parses from the same reads; clear_review and review_many are
    interleaved on both, and both are compared with each other and with Rings."""
    rr, cap = 3, 40
    res = {"input_calls": 0, "speak_calls": 0, "clears": 0, "reviews": 0, "lines_compared": 0, "n_bad": 0, "first_bad": [],
           "recorded": 0, "most_into_one_room_in_one_call": 0}
    ra, speakers, valid = levelled_roster(random.Random(seed), cap, review_rooms=rr)
    rb, speakers_b, valid_b = levelled_roster(random.Random(seed), cap, review_rooms=rr)
    assert valid == valid_b and speakers == speakers_b
    rng = random.Random(seed + 100)
    rings = Rings(rr)

    def review():
        rooms = list(range(rr))
        va, vb = ra.review_many(rooms), rb.review_many(rooms)
        for q in rooms:
            want = rings.lines(q)
            res["lines_compared"] += len(want)
            same = (va.lines(q) == vb.lines(q) == want and np.array_equal(va.stored[q], vb.stored[q])
                    and all(va.chunks(q, c) == vb.chunks(q, c) == rings.chunks(q, c) for c in (0, 1)))
            if not same:
                res["n_bad"] += 1
                res["first_bad"] += [{"room": q, "input": len(va.lines(q)), "speak": len(vb.lines(q)),
                                      "model": len(want)}][:5 - len(res["first_bad"])]
        res["reviews"] += 1

    with ra, rb:
        steps = ["input", "input", "clear", "review", "input_plain"] * 5 + ["input"] * 4
        rng.shuffle(steps)
        for op in steps + ["review"]:
            if op == "review":
                review()
            elif op == "clear":
                rooms = [rng.randrange(rr) for _ in range(rng.randint(1, 2))]
                for r in (ra, rb):
                    r.clear_review(rooms)
                for rm in rooms:
                    rings.clear(rm)
                res["clears"] += 1
            else:
                k = rng.choice((1, 7, 64, 200))
                ban = rng.random() < 0.5
                reads = [(rng.choice(valid), fuzz_read(rng)) for _ in range(k)]
                ra.input_many(reads, ban_swearing=ban, record=op == "input")
                res["input_calls"] += 1
                events, per_room = [], {}
                for slot, data in reads:
                    d, m = answer_of(speakers[slot], data, ban)
                    if d["kind"] == SPEECH and not d["forced"]:
                        events.append((slot, d["com"], data[d["start"]:d["start"] + d["size"]], d["word_count"]))
                    if op == "input" and m["recorded"]:
                        rings.record(m["rm"], m["line"])
                        per_room[m["rm"]] = per_room.get(m["rm"], 0) + 1
                        res["recorded"] += 1
                if events:
                    rb.speak_many(events, ban_swearing=ban, record=op == "input")
                    res["speak_calls"] += 1
                res["most_into_one_room_in_one_call"] = max([res["most_into_one_room_in_one_call"], *per_room.values()])
                if rng.random() < 0.5:
                    review()
    return res


def nothing_else_moved_part() -> dict:
    """broadcast_many, plan_many, speak_many and review_many give the same results and copy the same bytes before and
    after input_many calls and after an update of ``level``; input_many's upload depends on the reads alone."""
    out = {}
    rng = random.Random(11)
    roster, speakers, valid = levelled_roster(rng, 300, review_rooms=3)
    calls = [(b"Uaaa says: line %d ~FRred~RS\n" % i, rng.choice((None, 0, 1)), rng.choice((None, 5)), 0, SAY)
             for i in range(20)]
    events = [(rng.choice(valid), rng.choice(COMS), fuzz_inpstr(rng), rng.randrange(11)) for _ in range(100)]
    reads = [(rng.choice(valid), fuzz_read(rng)) for _ in range(200)]

    def snapshot():
        p, f = roster.plan_many(calls), roster.broadcast_many(calls)
        s, v = roster.speak_many(events, ban_swearing=True), roster.review_many([0, 1, 2])
        return {"plan": [p.admitted_bits.tobytes().hex()[:64], [p.variant(k, c).hex() for k in range(3) for c in (0, 1)],
                         p.variant_sizes.tolist(), p.write_counts.tolist(), int(p.admitted_bits.view(np.uint8).sum())],
                "fanout": [int(f.admitted.sum()), int(f.out_offsets[-1]), int(f.write_offsets[-1]),
                           f.arena[:2000].tobytes().hex()],
                "speak": [s.outcome.tolist(), s.text_sizes.tolist(), [s.line(k).hex() for k in range(10)],
                          s.room.variant_sizes.tolist(), s.reply.write_counts.tolist(),
                          int(s.room.admitted_bits.view(np.uint8).sum())],
                "review": [v.line_counts.tolist(), v.variant_sizes.tolist(), [x.hex() for x in v.lines(0)]],
                # plan, fanout, speak, review: [h2d, d2h] each
                "copies": [[r.timing["h2d_bytes"], r.timing["d2h_bytes"]] for r in (p, f, s, v)]}

    with roster:
        roster.plan_many(calls[:5], record=[c[1] is not None for c in calls[:5]])    # something in the rings
        snapshot()                                   # every kind of call once: the allocations have their sizes
        first = roster.input_many(reads).timing
        snapshot()
        out["before"] = snapshot()
        a = roster.input_many(reads).timing
        b = roster.input_many(reads, ban_swearing=True).timing
        out["after_input"] = snapshot()
        dirty_before = roster._dirty
        roster.update(valid[0], level=(speakers[valid[0]]["level"] + 1) % 5)
        out["level_update_left_dirty"] = [dirty_before, roster._dirty]
        out["after_level_update"] = snapshot()       # its speak_many, and it alone, uploads the speaker table once
        out["after_level_update_again"] = snapshot()
        c = roster.input_many(reads).timing
        roster.update(valid[0], level=speakers[valid[0]]["level"])
        d = roster.input_many(reads).timing
        e = roster.input_many(reads).timing
        out["after_input_again"] = snapshot()
        roster.update(valid[0], colour=1)
        g = roster.input_many(reads).timing
        out["input_h2d"] = {"first": first["h2d_bytes"], "clean": [a["h2d_bytes"], b["h2d_bytes"], c["h2d_bytes"], e["h2d_bytes"]],
                            "after_level_update": d["h2d_bytes"], "after_table_update": g["h2d_bytes"]}
        out["input_d2h"] = sorted({t["d2h_bytes"] for t in (first, a, b, c, d, e, g)})
        out["capacity"] = roster.capacity
    return out


def golden_part() -> dict:
    out = {}
    for name in GOLDEN:
        found: dict = {}
        res = replay_reads(name, device_answer(found))
        res["n_bad_vs_model"] = len(found.get("bad", []))
        res["first_bad_vs_model"] = found.get("bad", [])[:3]
        res["mismatches"] = res["mismatches"][:3]
        out[name] = res
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1733)
    a = ap.parse_args()
    out = {"device_count": device.device_count()}
    if out["device_count"] < 1:
        print("device_input_child: no GPU visible", file=sys.stderr)
        return 2
    out["golden"] = golden_part()
    out["fuzz"] = fuzz_part(a.seed)
    out["contract"] = contract_part(a.seed + 1)
    out["recording"] = recording_part(a.seed + 2)
    out["moved"] = nothing_else_moved_part()
    print("DEVICE_INPUT " + json.dumps(out, default=str))
    return 0


if __name__ == "__main__":
    sys.exit(main())
