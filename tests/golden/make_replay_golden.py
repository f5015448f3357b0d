#!/usr/bin/env python3
"""Generate tests/golden/reference_only/replay_<seed>.json: seeded random sessions, run against the REFERENCE build, for
tests/session_replay.py to replay through the Roster's calls.

    make -C oracle ref                           # needs the reference source (never on the GPU box)
    python tests/golden/make_replay_golden.py [--try SEED ...]

As make_who_golden.py: the scenarios are registered in this process only and recorded with ``run_scenario`` -- the
provisioning, the input lines and, per step, the bytes each client received --, ``long_date(1)`` in who()'s header is
replaced by the literal ``DATE``, and nothing is written unless the -O2 build, the -O0 build and a second run agree.

The sessions of ``session_replay.FIRST_SEEDS`` draw from the first command profile, described next.  Every other seed draws
from the second (below): the first profile's draws are untouched by it, so the first sessions regenerate byte for byte.

A session: four to six accounts of the levels NEW .. GOD with both colour bits, in every second session one in command
mode, in every fourth one muzzled, descriptions with ``~FBBM`` among them; ``max_clones`` 2; ``ban_swearing`` in every
second session.  Everybody logs in, then 60 line steps follow, drawn from the commands tests/session_replay.py answers
(speech in all its forms, tell and pemote at full names, prefixes, substrings, ``Nobody`` and oneself, ``.look``,
``.review`` with and without a room, ``.revtell``, ``.who``, what ends in ``Unknown command.``, ``.go``, the toggles,
``.vis`` / ``.invis``, ``.clone``, ``.destroy``, ``.chear``, ``.csay``).  The texts are
``random_text`` of tests/test_differential_fuzz.py.  The generator keeps a guess of where everybody's clones stand only
to aim ``.chear``, ``.csay`` and ``.destroy`` at them more often than chance would; what happened is the reference's word.

The second profile takes four steps in ten from ``second_line`` and the rest from the mix above: ``.public``, ``.private``,
``.letmein <room>`` and ``.invite <name>``, aimed by a guess of who stands where and which room is private; ``.rmst`` and
``.rmsn``; ``.desc``, ``.topic``, ``.inphr`` and ``.outphr`` with a text, without one and with one that is too long;
``.vis`` / ``.invis`` with a ``.go`` by the same user behind it; ``.go`` by a WIZ or above to a room that is not adjoined;
``.ignall`` twice by the same user, next to a clone of its own; ``.destroy <room> <name>`` by a GOD at an ARCH's clone; an
``.invite`` with the invited user's ``.go`` behind it; a third ``.clone``; once a session, a USER who walks to the corridor and
may not make it private alone, may with a second user there, says a line, and invites a third who was refused at the door;
and five lines that leave the clones' list order
different from their creation order, with a ``.look`` at them: a clone destroyed in front of another owner's, and a new one
created in that one's room.

Before it writes, the script replays every session through the CPU models (``session_replay.replay``) and asserts the
coverage tests/test_device_replay.py asserts again from the fixtures: every property of ``session_replay.COVERAGE`` is met
somewhere in the set, every step of every session is answered, and all five levels, both colour bits, a command
mode and a muzzled account are present.  ``--try`` records the given seeds without writing and prints what each covers:
that is how ``session_replay.SEEDS`` was chosen.
"""
from __future__ import annotations

import json
import random
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "tests" / "golden"))

from nuts333_amd import provision as pv                      # noqa: E402
from nuts333_amd.talker import REF_BINARY, REF_BINARY_O0    # noqa: E402
import scenarios                                            # noqa: E402
from scenario_runner import run_scenario                    # noqa: E402
from make_who_golden import _WHO_DATE                       # noqa: E402
from test_differential_fuzz import random_text              # noqa: E402
import session_replay                                       # noqa: E402

NAMES = ["Alice", "Bobby", "Carol", "Dave", "JoAnn", "Ann"]   # "ann" is Ann, behind JoAnn, who holds it; "oan" is JoAnn by strstr
KEYS = "abcdef"
ROOMS = ["drive", "hallway", "corridor", "lounge", "wizroom", "nowhere", "ha", "dr", "w", "co"]
DESCS = ["is here", "~FRis red", "is a plain user", "~OLbold~RS one", "~FBKcounts two"]
LINE_STEPS = 60
LINKS = {r.name: [x.name for x in pv.DEFAULT_ROOMS if x.label in r.links] for r in pv.DEFAULT_ROOMS}
SETTABLE = [r.name for r in pv.DEFAULT_ROOMS if r.access in ("", "BOTH")]          # the rooms .private and .public may change
# the texts the second profile sets: each ends in a plain word, which session_replay.last_word looks for in a listing
TEXTS = {".desc": ["~FGgreen~RS thumbs", "hums along", "is ~OLbold~RS today"], ".topic": ["the ~FRred~RS door", "nothing much", "who took the ~FYlast~RS biscuit"],
         ".inphr": ["tiptoes in", "~FMslides~RS over"], ".outphr": ["tiptoes off", "~FMslides~RS away"]}
TOO_LONG = "long " * 20                                                              # past USER_DESC_LEN, PHRASE_LEN and TOPIC_LEN
LONGEST_LINE = 700          # a broadcast and its relay prefix must fit the reference's text2[ARR_SIZE] (nuts333.c:1407)
OUT_DIR = Path(__file__).resolve().parent / "reference_only"
SIZE_LIMIT = (Path(__file__).resolve().parent / "vectors" / "transducer.json").stat().st_size


def make_accounts(seed: int, rng: random.Random) -> list:
    n = 4 + seed % 3
    levels = [1, rng.choice((0, 1, 2)), 2, 3, rng.choice((4, 4, 1)), rng.choice((0, 1, 3))][:n]
    accounts = []
    for i in range(n):
        desc = "~FBBMthree" if i == 2 else rng.choice(DESCS)
        accounts.append(pv.Account(NAMES[i], level=levels[i], colour=int(rng.random() < 0.5), desc=desc))
    if seed % 2:                                    # a WIZ at most in command mode: its prompt stays "COM> "
        accounts[1].command_mode, accounts[1].colour = 1, 0
    if seed % 4 == 2:
        accounts[0].muzzled = 2
    return accounts


def make_script(seed: int):
    rng = random.Random(seed)
    accounts = make_accounts(seed, rng)
    n = len(accounts)
    names = [a.name for a in accounts]
    colour = [bool(a.colour) for a in accounts]
    wizards = [i for i, a in enumerate(accounts) if a.level >= 3]
    guess = {i: [] for i in range(n)}               # where i's clones probably stand
    steps = []
    second = seed not in session_replay.FIRST_SEEDS
    where, private, asked = {i: "drive" for i in range(n)}, set(), set()     # the second profile's guesses: rooms, access, who typed .ignall
    partied, hidden = [], set()                     # who made the corridor private with company; who is probably invisible

    def went(i: int, room: str) -> str:
        """``.go room`` by i, and the guess of where that leaves it."""
        level = accounts[i].level
        if room in LINKS and (room in LINKS[where[i]] or level >= 2) and (room not in private or level >= 3) and (room != "wizroom" or level >= 2):
            where[i] = room
        return ".go " + room

    def second_line(i: int) -> list:
        """The next lines of the second profile, one to a dozen: a line is user i's, or ``(user, line)``."""
        here, level, x = where[i], accounts[i].level, rng.random()
        if x < 0.28:                                # moves: along a link towards the settable rooms, anywhere, nowhere
            y = rng.random()
            room = (rng.choice([r for r in LINKS[here] if r != "drive"] or LINKS[here]) if y < 0.55 else rng.choice(SETTABLE) if y < 0.8
                    else here if y < 0.9 else rng.choice(ROOMS))
            lines = []
            if level >= 3 and rng.random() < 0.35:
                turn = rng.random() < 0.8           # mostly the one of the two that takes effect
                lines = [".vis" if (i in hidden) == turn else ".invis"]
                if turn:
                    hidden.symmetric_difference_update({i})
            return lines + [went(i, room)]
        if x < 0.56:                                # access
            y = rng.random()
            locked = [r for r in LINKS[here] if r in private]
            users = [k for k in range(n) if accounts[k].level == 1]
            guests = [k for k in range(n) if accounts[k].level in (1, 2) and k not in users[:1]]
            if "corridor" not in private and not partied and users and guests and y < 0.5:
                # a USER alone in the corridor may not make it private; with a second user it may; a third is refused at the
                # door, invited, and walks in
                p, g = users[0], rng.choice(guests)
                h = rng.choice([k for k in range(n) if k not in (p, g) and accounts[k].level >= 1])
                walk = lambda k, to: [(k, went(k, room)) for room in {"drive": ["hallway", "corridor"], "wizroom": ["hallway", "corridor"],
                                                                      "corridor": []}.get(where[k], ["corridor"])[:to]]
                lines = (walk(p, 2) + [(p, ".private")] + walk(h, 2) + [(p, ".private"), (p, ".say " + random_text(rng)[:60])] + walk(g, 1)
                         + [(g, ".go corridor"), (p, ".invite " + names[g].lower()), (g, ".go corridor")])
                private.add("corridor")
                partied.append(p)
                where[g] = "corridor"
                return lines
            if y < 0.12:
                return [rng.choice([".public", ".invite", ".letmein", ".invite nobody", ".letmein drive", ".private drive", ".private nowhere",
                                    ".letmein " + rng.choice(ROOMS)])]
            if locked and y < 0.6:
                return [".letmein " + rng.choice(locked)]
            if here in private:
                if y < 0.75:                        # an invitation, and half of the time the invited on its way at once
                    k = rng.choice([k for k in range(n) if where[k] in LINKS[here]] or [k for k in range(n) if where[k] != here] or [i])
                    return [".invite " + names[k].lower()] + ([(k, went(k, here))] if rng.random() < 0.5 else [])
                private.discard(here)
                return [".public"]
            if here in SETTABLE or level >= 3 and y < 0.5:
                room = here if here in SETTABLE else rng.choice(SETTABLE)
                if level >= 2 or sum(w == room for w in where.values()) >= 2:
                    private.add(room)
                return [".private" if room == here else ".private " + room]
            return [went(i, rng.choice(SETTABLE + LINKS[here]))]
        if x < 0.64:
            return [rng.choice([".rmst", ".rmsn"])]
        if x < 0.86:                                # what a user sets of its own
            com, y = rng.choice(list(TEXTS)), rng.random()
            return [com if y < 0.2 else com + " " + TOO_LONG if y < 0.32 else com + " " + rng.choice(TEXTS[com])]
        if wizards and rng.random() < 0.7:          # next to a clone of one's own; a GOD at an ARCH's clone
            i = rng.choice(wizards)
            gods = [k for k in wizards if accounts[k].level == 4]
            theirs = [(k, room) for k in wizards if accounts[k].level == 3 for room in guess[k]]
            if gods and theirs and rng.random() < 0.4:
                k, room = rng.choice(theirs)
                guess[k].remove(room)
                return [(gods[0], ".destroy " + room + " " + names[k].lower())]
            others = [k for k in wizards if k != i and len(guess[k]) < 2 and where[i] not in guess[k]]
            if others and not guess[i] and where[i] != "corridor" and rng.random() < 0.5:
                # a record destroyed in front of another's, and a new one in that one's room: list order is not creation order
                k, room = rng.choice(others), where[i]
                guess[k].append(room)
                guess[i].append(room)
                looker = rng.choice([j for j in range(n) if where[j] == room] or [i])
                return [(i, ".clone corridor"), (k, ".clone " + room), (i, ".destroy corridor"), (i, ".clone " + room), (looker, ".look")]
            if len(guess[i]) >= 2:
                return [(i, ".clone " + rng.choice(SETTABLE))]
            if where[i] not in guess[i]:
                guess[i].append(where[i])
                return [(i, ".clone"), (i, ".ignall")]
            return [(i, ".ignall")]
        if i in asked:
            asked.discard(i)
        else:
            asked.add(i)
        return [".ignall"] + ([(rng.choice(sorted(asked)), ".ignall")] if asked and rng.random() < 0.5 else [])

    def target() -> str:
        name = rng.choice(names)
        x = rng.random()
        if x < 0.35:
            return name.lower()
        if x < 0.55:
            return name[:rng.randint(2, 3)].lower()
        if x < 0.8:
            a = rng.randrange(1, len(name) - 1)
            return name[a:a + rng.randint(2, 3)].lower()
        return rng.choice(["Nobody", "nobody", "zz"])

    while len(steps) < LINE_STEPS:
        i = rng.randrange(n)
        if second and rng.random() < 0.4:
            for line in second_line(i):
                k, line = line if isinstance(line, tuple) else (i, line)
                steps.append((KEYS[k], line, {}))
            continue
        r = rng.random()
        flags = {}
        if r < 0.21:
            text = random_text(rng)
            line = text if text[0] not in ".;!<>-#" else "x" + text
            if accounts[i].command_mode:
                line = ".say " + line
        elif r < 0.27:
            line = rng.choice([".shout ", "! ", ".sh "]) + random_text(rng)
        elif r < 0.34:
            line = rng.choice([";", ".emote ", "#", ".semote "]) + random_text(rng)
        elif r < 0.45:
            who = names[i].lower() if rng.random() < 0.08 else target()
            line = rng.choice([".tell ", "> "]) + who + " " + random_text(rng)
        elif r < 0.51:
            who = names[i].lower() if rng.random() < 0.08 else target()
            line = rng.choice(["< ", ".pemote "]) + who + " " + random_text(rng)
        elif r < 0.545:
            line = ".look"
        elif r < 0.595:
            line = rng.choice([".review", ".review", ".rev " + rng.choice(ROOMS), ".review " + rng.choice(ROOMS)])
        elif r < 0.635:
            line = ".revtell"
        elif r < 0.67:
            line = ".who"
        elif r < 0.71:
            line = rng.choice([".bogus", ".say", ".tell", ".xyzzy now"])
        elif r < 0.80:
            line = ".go " + (rng.choice(ROOMS) if rng.random() < 0.4 else rng.choice(["hallway", "hallway", "drive", "corridor", "ha"]))
        elif r < 0.86:
            line = rng.choice([".ignall", ".ignshout", ".ignshout", ".igntell", ".igntell", ".colour"])
            if line == ".colour":
                if accounts[i].command_mode:
                    continue
                colour[i] = not colour[i]
                flags = {"colour": colour[i]}
        else:                                       # the commands of an ARCH, mostly from one
            if wizards and rng.random() < 0.9:
                i = rng.choice(wizards)
            mine = guess[i]
            room = rng.choice(mine) if mine and rng.random() < 0.75 else rng.choice(["drive", "drive", "hallway", "hallway", "corridor", "lounge"])
            x = rng.random()
            if x < 0.12:
                line = rng.choice([".vis", ".invis", ".invis"])
            elif x < 0.42:
                line = ".clone " + room if rng.random() < 0.8 else ".clone"
                if room not in mine and len(mine) < 2 and line != ".clone":
                    mine.append(room)
            elif x < 0.52:
                line = ".destroy " + room + (" " + rng.choice(names).lower() if rng.random() < 0.2 else "")
                if room in mine and line.endswith(room):
                    mine.remove(room)
            elif x < 0.78:
                line = ".chear " + room + " " + rng.choice(["all", "swears", "swears", "nothing", "nothing", "some"])
            else:
                line = ".csay " + room + " " + random_text(rng)
        steps.append((KEYS[i], line[:LONGEST_LINE], flags))

    del steps[LINE_STEPS:]

    def script(s):
        for k, a in zip(KEYS, accounts):
            s.connect(k)
            s.login(k, a.name, colour=bool(a.colour), sync_suffix=b"COM> " if a.command_mode else b"")
        for k, line, flags in steps:
            s.line(k, line, **flags)

    return {"ban_swearing": seed % 2 == 0, "max_clones": 2}, accounts, script


def record(seed: int, binary) -> dict:
    """Session ``seed`` recorded against ``binary``; the scenario is registered for the length of the call."""
    name = f"replay_{seed}"
    scenarios.REFERENCE_ONLY[name] = lambda: make_script(seed)
    try:
        out = run_scenario(name, binary)
    finally:
        del scenarios.REFERENCE_ONLY[name]
    for st in out["steps"]:
        st["recv"] = {k: _WHO_DATE.sub(r"\1DATE\2", v) for k, v in st["recv"].items()}
    return out


def render(doc: dict) -> str:
    return json.dumps(doc, indent=1, ensure_ascii=True) + "\n"


def stable(seed: int):
    a = record(seed, REF_BINARY)
    if REF_BINARY_O0.exists() and a != record(seed, REF_BINARY_O0):
        raise SystemExit(f"replay_{seed}: -O2 and -O0 reference builds disagree")
    if a != record(seed, REF_BINARY):
        raise SystemExit(f"replay_{seed}: two runs of the same build disagree (nondeterministic capture)")
    return a


def main(argv) -> int:
    if not REF_BINARY.exists():
        print("oracle/_ref/nuts333 is missing: run `make -C oracle ref` first", file=sys.stderr)
        return 2
    if argv and argv[0] == "--try":
        for seed in map(int, argv[1:]):
            try:
                doc = record(seed, REF_BINARY)
                res = session_replay.replay(doc)
            except Exception as e:                  # a seed that types something the replayer does not answer
                print(seed, "unusable:", repr(e)[:200])
                continue
            print(seed, f"answered {res['answered']} tracked {res['tracked']}", f"mismatches {len(res['mismatches'])}", f"bytes {len(render(doc))}",
                  " ".join(f"{k}={v}" for k, v in res["coverage"].items() if v), sorted({a["level"] for a in doc["accounts"][0]}))
            for m in res["mismatches"][:2]:
                print("   ", m)
        return 0
    docs = {seed: stable(seed) for seed in session_replay.SEEDS}
    missing = session_replay.coverage_gaps(docs)
    if missing:
        print("the sessions do not cover what they must:\n  " + "\n  ".join(missing), file=sys.stderr)
        return 1
    for seed, doc in docs.items():
        text = render(doc)
        if len(text) >= SIZE_LIMIT:
            print(f"replay_{seed}: {len(text)} bytes, the limit is {SIZE_LIMIT}", file=sys.stderr)
            return 1
        path = OUT_DIR / f"replay_{seed}.json"
        path.write_text(text)
        print(f"replay_{seed}: {len(doc['steps'])} steps, {len(text)} bytes -> {path.relative_to(REPO)}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
