#!/usr/bin/env python3
"""Generate tests/golden/reference_only/set.json: a session about the commands a user sets its own state with -- ``.mode``,
``.ignall``, ``.prompt``, ``.desc``, ``.inphr``, ``.outphr``, ``.topic``, ``.vis``, ``.invis``, ``.charecho``, ``.afk``,
``.colour``, ``.ignshout`` and ``.igntell`` -- run against the REFERENCE build.

    make -C oracle ref                           # needs the reference source (never on the GPU box)
    python tests/golden/make_set_golden.py

As make_clone_golden.py: one single-talker scenario of its own, registered in its own process.  The -O2 and the -O0
reference builds, and two runs of the same build, must give the same fixture; the script checks that before it writes.

Four accounts, all in the drive: Alice, a USER with colour; Bobby, a plain USER; Carol, a plain USER who ignores everyone
for most of the session; Dave, an ARCH with colour, invisible for a part of it.

The prompt of a user outside command mode holds the time of day, so ``.prompt`` is toggled inside command mode alone,
where ``prompt()`` writes ``COM> `` and returns (nuts333.c:2185-2188).  A client that is AFK cannot take part in the
round trips that end a step; whatever it types next comes back first (nuts333.c:180-203), and since that return clears
``afk_mesg`` a single talker never reaches an ``.afk`` that finds a message kept from before: that branch is left to the
seeded streams and the hand-built rosters of tests/test_device_set.py.

What the session holds, each under a ``note`` of its own: the six toggles both ways, ``.ignall`` by an invisible ARCH,
the listener who ignores everyone; ``.colour`` on by a user whose colour was off, off again, and the video test; ``.vis``
and ``.invis`` in all four branches; ``.desc`` queried, of 30 and of 31 bytes, with ``(CLONE)`` inside the first word and
in the second word only; both phrases queried, of 40 and of 41 bytes, and used by a ``.go``; the topic queried without
and with a topic, of 60 and of 61 bytes, and set by an invisible actor; ``.afk`` bare, with a message, locked, locked
with a message, by an invisible user, and with a 61-byte message with and without ``lock``.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from nuts333_amd import provision as pv                      # noqa: E402
from nuts333_amd.talker import REF_BINARY, REF_BINARY_O0    # noqa: E402
import scenarios                                            # noqa: E402
from scenario_runner import run_scenario                    # noqa: E402

CONFIG = {"max_clones": 1}
DESC30, PHRASE40, TOPIC60, MESG60 = "d" * 26 + " end", "strides in with forty bytes of a phrase!", "t" * 55 + " done", "m" * 56 + " brb"
assert (len(DESC30), len(PHRASE40), len(TOPIC60), len(MESG60)) == (30, 40, 60, 60)
#: note -> what the actor's own bytes must hold
WANTED = {
    "ignshout on": "You are now ignoring shouts and shout emotes.", "ignshout off": "You are no longer ignoring shouts and shout emotes.",
    "igntell on": "You are now ignoring tells and private emotes.", "igntell off": "You are no longer ignoring tells and private emotes.",
    "charecho on": "Echoing for character mode clients \x1b[32mON.", "charecho off": "Echoing for character mode clients \x1b[31mOFF.",
    "ignall on": "You are now ignoring everyone.", "ignall off": "You will now hear everyone again.",
    "the listener who ignores everyone": "You are now ignoring everyone.",
    "colour on by a user whose colour was off": "Colour \x1b[32mON.", "colour off": "Colour \x1b[31mOFF.",
    "mode command": "Now in COMMAND mode.", "prompt on": "Prompt \x1b[32mON.", "prompt off": "Prompt \x1b[31mOFF.",
    "the video test": "BW: \x1b[47mNUTS 3 VIDEO TEST", "mode speech": "Now in SPEECH mode.",
    "topic query with no topic": "No topic has been set yet.", "a topic of 60 bytes": "Topic set to: " + TOPIC60,
    "topic query": "The current topic is: " + TOPIC60, "a topic of 61 bytes": "Topic too long.",
    "vis when visible": "You are already visible.", "became invisible": "You recite a melodic incantation and fade out.",
    "invis when invisible": "You are already invisible.", "ignall by an invisible ARCH": "You are now ignoring everyone.",
    "topic by an invisible actor": "Topic set to: under the radar", "afk by an invisible user": "You are now AFK, press <return> to reset.",
    "became visible": "You recite a melodic incantation and reappear.",
    "desc query": "Your current description is: is a bot", "a desc of 30 bytes": "Description set.", "a desc of 31 bytes": "Description too long.",
    "(CLONE) inside the first word": "You cannot have that description.", "(CLONE) in the second word only": "Description set.",
    "inphr query": "Your current in phrase is: enters", "an in phrase of 40 bytes": "In phrase set.", "an in phrase of 41 bytes": "Phrase too long.",
    "outphr query": "Your current out phrase is: goes", "an out phrase of 40 bytes": "Out phrase set.",
    "an out phrase of 41 bytes": "Phrase too long.", "inphr query after": "Your current in phrase is: " + PHRASE40,
    "afk": "You are now AFK, press <return> to reset.", "afk with a message": "AFK message set.",
    "afk lock": "You are now AFK with the session locked, enter your password to unlock it.",
    "afk lock with a message": "AFK message set.", "a 61-byte message": "AFK message too long.",
    "a 61-byte message with lock": "AFK message too long.", "a 60-byte message with lock": "AFK message set.",
}
#: (note, client, needle): what somebody else must have been sent
HEARD = (
    ("ignall on", "b", "Alice is now ignoring everyone."), ("ignall off", "d", "Alice is listening again."),
    ("ignall by an invisible ARCH", "b", "Dave is now ignoring everyone."), ("became invisible", "b", "Dave recites a melodic incantation and disappears!"),
    ("became visible", "a", "You hear a melodic incantation chanted and Dave materialises!"),
    ("topic by an invisible actor", "b", "A presence has set the topic to: under the radar"),
    ("a topic of 60 bytes", "a", "Bobby has set the topic to: " + TOPIC60),
    ("afk", "b", "Alice goes AFK..."), ("afk with a message", "b", "Alice goes AFK: gone for tea"),
    ("afk lock", "b", "Alice goes AFK..."), ("afk lock with a message", "d", "Alice goes AFK: back at ten"),
    ("a 60-byte message with lock", "b", "Alice goes AFK: " + MESG60), ("a tell to the AFK user", "b", "Alice is AFK, message is: gone for tea"),
    ("the phrases at work", "b", "Alice " + PHRASE40 + "."),
)
#: (note, client, needle): what somebody must not have been sent
UNHEARD = (("ignall on", "c", "Alice"), ("became invisible", "c", "Dave"), ("afk by an invisible user", "b", "AFK"),
           ("afk with a message", "c", "Alice"), ("a 61-byte message", "b", "AFK"))


def settings():
    accounts = [pv.Account("Alice", level=1, colour=1), pv.Account("Bobby", level=1), pv.Account("Carol", level=1),
                pv.Account("Dave", level=3, colour=1)]

    def configs(p):
        return [pv.TalkerConfig(mainport=p[0][0], wizport=p[0][1], linkport=p[0][2], max_users=50)]

    def script(s):
        for k, a in zip("abcd", accounts):
            s.connect(k); s.login(k, a.name, colour=bool(a.colour))
        # -- the toggles
        s.line("a", ".ignshout", note="ignshout on")
        s.line("a", ".ignshout", note="ignshout off")
        s.line("a", ".igntell", note="igntell on")
        s.line("a", ".igntell", note="igntell off")
        s.line("a", ".charecho", note="charecho on")
        s.line("a", ".charecho", note="charecho off")
        s.line("c", ".ignall", note="the listener who ignores everyone", hears_broadcasts=False)
        s.line("a", ".ignall", note="ignall on", hears_broadcasts=False)
        s.line("b", "a line Alice does not hear")
        s.line("a", ".ignall", note="ignall off", hears_broadcasts=True)
        # -- .colour, .mode, .prompt and the video test
        s.line("b", ".colour", colour=True, note="colour on by a user whose colour was off")
        s.line("b", "a line with ~FRcolour")
        s.line("b", ".colour", colour=False, note="colour off")
        s.line("a", ".mode", sync_suffix=b"\x1b[36mCOM> \x1b[0m", note="mode command")       # Alice has colour
        s.line("a", ".prompt", note="prompt on")
        s.line("a", "prompt", note="prompt off")
        s.line("a", ".ignall", hears_broadcasts=False)
        s.line("a", ".charecho")
        s.line("a", ".colour", note="the video test")
        s.line("a", ".charecho")
        s.line("a", ".ignall", hears_broadcasts=True)
        s.line("a", ".mode", sync_suffix=b"", note="mode speech")
        # -- .topic
        s.line("b", ".topic", note="topic query with no topic")
        s.line("b", ".topic " + TOPIC60, note="a topic of 60 bytes")
        s.line("b", ".topic", note="topic query")
        s.line("b", ".topic " + TOPIC60 + "x", note="a topic of 61 bytes")
        s.line("a", ".look")
        # -- .vis and .invis, and what an invisible ARCH does
        s.line("d", ".vis", note="vis when visible")
        s.line("d", ".invis", note="became invisible")
        s.line("d", ".invis", note="invis when invisible")
        s.line("d", ".ignall", note="ignall by an invisible ARCH", hears_broadcasts=False)
        s.line("d", ".ignall", hears_broadcasts=True)
        s.line("d", ".topic under the radar", note="topic by an invisible actor")
        s.line("d", ".afk", can_sync=False, note="afk by an invisible user")
        s.line("d", "", can_sync=True, note="an invisible user comes back")
        s.line("d", ".vis", note="became visible")
        # -- .desc
        s.line("a", ".desc", note="desc query")
        s.line("a", ".desc " + DESC30, note="a desc of 30 bytes")
        s.line("a", ".desc " + DESC30 + "x", note="a desc of 31 bytes")
        s.line("a", ".desc the(CLONE)one", note="(CLONE) inside the first word")
        s.line("a", ".desc a (CLONE)", note="(CLONE) in the second word only")
        s.line("b", ".look")
        s.line("a", ".desc", note="desc query after")
        # -- the phrases
        s.line("a", ".inphr", note="inphr query")
        s.line("a", ".inphr " + PHRASE40, note="an in phrase of 40 bytes")
        s.line("a", ".inphr " + PHRASE40 + "x", note="an in phrase of 41 bytes")
        s.line("a", ".outphr", note="outphr query")
        s.line("a", ".outphr " + PHRASE40[::-1], note="an out phrase of 40 bytes")
        s.line("a", ".outphr " + PHRASE40 + "x", note="an out phrase of 41 bytes")
        s.line("a", ".inphr", note="inphr query after")
        s.line("a", ".go hallway")
        s.line("a", ".go drive", note="the phrases at work")
        # -- .afk
        s.line("a", ".afk", can_sync=False, note="afk")
        s.line("a", "back with a line of speech", can_sync=True, note="the return, then the line")
        s.line("a", ".afk gone for tea", can_sync=False, note="afk with a message")
        s.line("b", ".tell alice are you there", note="a tell to the AFK user")
        s.line("a", "", can_sync=True, note="an empty line is enough")
        s.line("a", ".afk lock", can_sync=False, note="afk lock")
        s.line("a", "test", expect=b"no longer AFK.\x1b[0m\n\r\x1b[0m", can_sync=True, note="unlocked")
        s.line("a", ".afk lock back at ten", can_sync=False, note="afk lock with a message")
        s.line("a", "test", expect=b"no longer AFK.\x1b[0m\n\r\x1b[0m", can_sync=True)
        s.line("a", ".afk " + MESG60 + "x", note="a 61-byte message")
        s.line("a", ".afk lock " + MESG60 + "x", note="a 61-byte message with lock")
        s.line("a", ".afk lock " + MESG60, can_sync=False, note="a 60-byte message with lock")
        s.line("a", "test", expect=b"no longer AFK.\x1b[0m\n\r\x1b[0m", can_sync=True)
        s.line("a", ".afk lockx", can_sync=False, note="a word that is not lock")
        s.line("a", "", can_sync=True)

    return {"configs": configs, "accounts": [accounts], "boot_order": [0], "script": script, "config_kw": CONFIG}


def main() -> int:
    scenarios.REFERENCE_ONLY["set"] = settings
    if not REF_BINARY.exists():
        print("oracle/_ref/nuts333 is missing: run `make -C oracle ref` first", file=sys.stderr)
        return 2
    a = run_scenario("set", REF_BINARY)
    b = run_scenario("set", REF_BINARY_O0) if REF_BINARY_O0.exists() else a
    if a != b:
        print("set: -O2 and -O0 reference builds disagree", file=sys.stderr)
        return 1
    if a != run_scenario("set", REF_BINARY):
        print("set: two runs of the same build disagree (nondeterministic capture)", file=sys.stderr)
        return 1
    by_note = {st.get("note"): st for st in a["steps"] if st.get("note")}
    missing = [note for note, needle in WANTED.items() if needle not in by_note.get(note, {"recv": {}, "actor": ""})["recv"].get(
        by_note.get(note, {"actor": ""})["actor"], "")]
    missing += [f"{note} ({client})" for note, client, needle in HEARD if needle not in by_note[note]["recv"].get(client, "")]
    missing += [f"{note} ({client}, not)" for note, client, needle in UNHEARD if needle in by_note[note]["recv"].get(client, "")]
    if missing:
        print(f"set: steps that did not go as the session claims: {missing}", file=sys.stderr)
        for note in missing:
            st = by_note.get(note.split(" (")[0])
            print(note, "->", st and st["recv"], file=sys.stderr)
        return 1
    path = Path(__file__).resolve().parent / "reference_only" / "set.json"
    path.write_text(json.dumps(a, indent=1, ensure_ascii=True) + "\n")
    lines = sum(1 for st in a["steps"] if st["op"] == "line")
    print(f"set: {len(a['steps'])} steps, {lines} of them lines -> {path.relative_to(REPO)}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
