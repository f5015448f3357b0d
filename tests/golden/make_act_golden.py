#!/usr/bin/env python3
"""Generate tests/golden/reference_only/act.json: a session of the commands a user aims at another user -- ``.move``,
``.wake``, ``.muzzle`` and ``.unmuzzle`` -- run against the REFERENCE build.

    make -C oracle ref                           # needs the reference source (never on the GPU box)
    python tests/golden/make_act_golden.py

As make_access_golden.py: one single-talker scenario of its own, registered in its own process.  The -O2 and the -O0
reference builds, and two runs of the same build, must give the same fixture; the script checks that before it writes.
The talker runs with ``min_private 2``, ``ignore_mp_level WIZ`` and ``gatecrash_level ARCH``, as every provisioned config
does, and ``max_clones 1``, over the shipped five rooms.

Five accounts: Alice, a USER with colour; Bobby, a plain USER; Carol, a WIZ; Dave, an ARCH with colour, who goes
``.invis`` and ``.clone``s; Gina, a GOD.

What the session holds, for tests/test_device_act.py, each under a ``note`` of its own.  ``.move``: every refusal (usage,
nobody, no such room, oneself, the level, already there, private to the actor); a move out of the actor's room, whose target
hears the chant line and then the giant hand; a move into the actor's own room without a word, whose actor hears the
enter line after its reply; a move into a private room by the actor's level and one by the actor's invitation; a move that
clears the target's invitation, shown by the ``.go`` that is refused afterwards; a move out of a private room that thereby
returns to public, with the ``.review`` of the room afterwards, which is empty; a move by an invisible actor; a move of an
invisible target; a move past a clone that relays; a listener with ``ignall``.  ``.wake``: usage, nobody, oneself, woken,
woken by an invisible actor, a user who is AFK (the ``.afk`` before it and the return from it after it are steps of the
session that change the state and are not answered: they are ``set_many``'s and the caller's), and a muzzled user's wake
refused.  ``.muzzle`` and ``.unmuzzle``: usage, oneself, the level,
muzzled by the WIZ, already muzzled, muzzled again by the ARCH (a second level), the WIZ's ``.unmuzzle`` refused as above
its level, the muzzled user's say refused, unmuzzled by the ARCH, the silent ``.unmuzzle`` of a user who is not muzzled,
and the two branches for a name that is not logged on, which the reference answers from the user file.

NOT in the session: ACT_MOVE_AWAY, the release of a user who stands in no room, which needs a second talker and a netlink.
That branch composes nothing and is held to the model alone (tests/test_device_act.py).
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

CONFIG = {"max_clones": 1, "min_private": 2, "ignore_mp_level": 2, "gatecrash_level": 3}
CHANT = "You chant an ancient spell..."
#: note -> what the actor's own bytes must hold
WANTED = {
    "move usage": "Usage: move <user> [<room>]", "move nobody": "There is no one of that name logged on.",
    "move no such room": "There is no such room.", "move oneself": "Trying to move yourself this way is the fourth sign of madness.",
    "move the level": "You cannot move a user of equal or higher level than yourself.", "move already": "Alice is already in the drive.",
    "move refused as private": "The corridor is currently private, Alice cannot be moved there.",
    "out of the actor's room": CHANT, "into the actor's own room": CHANT, "into a private room by level": CHANT,
    "an invitation for the WIZ": "You invite Carol in.", "into a private room by invitation": CHANT,
    "the room returns to public": CHANT, "the buffer is empty": "Review buffer is empty.",
    "an invitation for the target": "You invite Bobby in.", "the target's invitation is cleared": CHANT,
    "the invitation is gone": "That room is currently private, you cannot enter.",
    "an invisible actor": CHANT, "an invisible target": CHANT, "past a clone that relays": CHANT, "an ignall listener": CHANT,
    "wake usage": "Usage: wake <user>", "wake nobody": "There is no one of that name logged on.",
    "wake oneself": "Trying to wake yourself up is the eighth sign of madness.", "woken": "Wake up call sent.",
    "woken by an invisible actor": "Wake up call sent.", "wake AFK": "You cannot wake someone who is AFK.",
    "muzzle usage": "Usage: muzzle <user>", "muzzle oneself": "Trying to muzzle yourself is the ninth sign of madness.",
    "muzzle the level": "You cannot muzzle a user of equal or higher level than yourself.",
    "muzzled by the WIZ": "Alice now has a muzzle of level: WIZ.", "already muzzled": "Alice is already muzzled.",
    "muzzled by the ARCH": "Alice now has a muzzle of level: ", "unmuzzle above the level": "Alice's muzzle is set to level ARCH, you do not have the power to remove it.",
    "a muzzled say": "You are muzzled, you cannot speak.", "a muzzled wake": "You are muzzled, you cannot wake anyone.",
    "unmuzzled": "You remove Alice's muzzle.", "unmuzzle usage": "Usage: unmuzzle <user>",
    "unmuzzle oneself": "Trying to unmuzzle yourself is the tenth sign of madness.", "not muzzled: nothing is written": "",
    "muzzle absent": "There is no such user.", "unmuzzle absent": "There is no such user.",
}
#: (note, client, needle): what somebody else must have been sent
HEARD = (
    ("out of the actor's room", "c", "Dave chants an ancient spell..."),
    ("out of the actor's room", "c", "A giant hand grabs you and pulls you into a magical blue vortex!"),
    ("out of the actor's room", "a", "A giant hand grabs Carol who is pulled into a magical blue vortex!"),
    ("into the actor's own room", "d", "Carol falls out of a magical blue vortex!"),
    ("the room returns to public", "a", "Room access returned to "),
    ("an invisible actor", "c", "A presence chants an ancient spell..."),
    ("an invisible target", "b", "A presence leaves the room."),
    ("past a clone that relays", "d", "[ hallway ]:"),
    ("woken", "b", "Alice says: "), ("woken by an invisible actor", "a", "A presence says: "),
    ("muzzled by the WIZ", "a", "You have been muzzled!"), ("unmuzzled", "a", "You have been unmuzzled!"),
)
#: the steps at which somebody must have been sent nothing at all
SILENT = (("not muzzled: nothing is written", "c"), ("an ignall listener", "b"))


def act():
    accounts = [pv.Account("Alice", level=1, colour=1), pv.Account("Bobby", level=1), pv.Account("Carol", level=2),
                pv.Account("Dave", level=3, colour=1), pv.Account("Gina", level=4)]

    def configs(p):
        return [pv.TalkerConfig(mainport=p[0][0], wizport=p[0][1], linkport=p[0][2], max_users=50, max_clones=1)]

    def script(s):
        for k, a in zip("abcde", accounts):
            s.connect(k); s.login(k, a.name, colour=bool(a.colour))
        # -- .move: the refusals
        s.line("c", ".move", note="move usage")
        s.line("c", ".move nobody", note="move nobody")
        s.line("c", ".move alice nosuch", note="move no such room")
        s.line("c", ".move carol", note="move oneself")
        s.line("c", ".move dave hallway", note="move the level")
        s.line("c", ".move ali", note="move already")
        s.line("d", ".private corridor")
        s.line("c", ".move alice corridor", note="move refused as private")
        # -- .move: the moves
        s.line("d", ".move carol hallway", note="out of the actor's room")
        s.line("d", ".move carol", note="into the actor's own room")
        s.line("d", ".move alice corr", note="into a private room by level")
        s.line("a", "a line for the review buffer")
        s.line("a", ".invite carol", note="an invitation for the WIZ")
        s.line("c", ".move bobby corridor", note="into a private room by invitation")
        s.line("d", ".move bobby", note="the room returns to public")
        s.line("a", ".review", note="the buffer is empty")
        s.line("d", ".private corridor")
        s.line("e", ".go hallway")
        s.line("e", ".go corridor")
        s.line("a", ".invite bobby", note="an invitation for the target")
        s.line("d", ".move bobby corridor", note="the target's invitation is cleared")
        s.line("b", ".go hallway")
        s.line("b", ".go corridor", note="the invitation is gone")
        s.line("d", ".invis")
        s.line("d", ".move bobby", note="an invisible actor")
        s.line("e", ".move dave hallway", note="an invisible target")
        s.line("d", ".go drive")
        s.line("d", ".clone hallway")
        s.line("d", ".move carol hallway", note="past a clone that relays")
        s.line("b", ".ignall")
        s.line("d", ".move carol", note="an ignall listener")
        s.line("b", ".ignall")
        s.line("d", ".destroy hallway")
        # -- .wake
        s.line("a", ".wake", note="wake usage")
        s.line("a", ".wake nobody", note="wake nobody")
        s.line("a", ".wake alice", note="wake oneself")
        s.line("a", ".wake bob", note="woken")
        s.line("d", ".wake alice", note="woken by an invisible actor")
        s.line("b", ".afk", can_sync=False, note="a user goes AFK")
        s.line("a", ".wake bobby", note="wake AFK")
        s.line("b", "back again", can_sync=True, note="the return from AFK")
        # -- .muzzle and .unmuzzle
        s.line("c", ".muzzle", note="muzzle usage")
        s.line("c", ".muzzle carol", note="muzzle oneself")
        s.line("c", ".muzzle dave", note="muzzle the level")
        s.line("c", ".muzzle alice", note="muzzled by the WIZ")
        s.line("c", ".muzzle alice", note="already muzzled")
        s.line("d", ".muzzle alice", note="muzzled by the ARCH")
        s.line("c", ".unmuzzle alice", note="unmuzzle above the level")
        s.line("a", "a muzzled user says this", note="a muzzled say")
        s.line("a", ".wake bobby", note="a muzzled wake")
        s.line("d", ".unmuzzle ali", note="unmuzzled")
        s.line("a", "and speaks again")
        s.line("c", ".unmuzzle", note="unmuzzle usage")
        s.line("c", ".unmuzzle carol", note="unmuzzle oneself")
        s.line("c", ".unmuzzle bobby", note="not muzzled: nothing is written")
        s.line("c", ".muzzle nosuchuser", note="muzzle absent")
        s.line("c", ".unmuzzle nosuchuser", note="unmuzzle absent")

    return {"configs": configs, "accounts": [accounts], "boot_order": [0], "script": script, "config_kw": CONFIG}


def main() -> int:
    scenarios.REFERENCE_ONLY["act"] = act
    if not REF_BINARY.exists():
        print("oracle/_ref/nuts333 is missing: run `make -C oracle ref` first", file=sys.stderr)
        return 2
    a = run_scenario("act", REF_BINARY)
    b = run_scenario("act", REF_BINARY_O0) if REF_BINARY_O0.exists() else a
    if a != b:
        print("act: -O2 and -O0 reference builds disagree", file=sys.stderr)
        return 1
    if a != run_scenario("act", REF_BINARY):
        print("act: two runs of the same build disagree (nondeterministic capture)", file=sys.stderr)
        return 1
    by_note = {st.get("note"): st for st in a["steps"] if st.get("note")}
    mine = lambda note: by_note[note]["recv"].get(by_note[note]["actor"], "") if note in by_note else None
    missing = [note for note, needle in WANTED.items() if mine(note) is None or needle not in mine(note) or (not needle and mine(note))]
    missing += [f"{note} ({client})" for note, client, needle in HEARD if needle not in by_note[note]["recv"].get(client, "")]
    missing += [f"{note} ({client} is not silent)" for note, client in SILENT if by_note[note]["recv"].get(client, "")]
    if "giant hand" in by_note["an invisible target"]["recv"].get("d", ""):
        missing.append("an invisible target (it was sent the giant hand)")
    if missing:
        print(f"act: steps that did not go as the session claims: {missing}", file=sys.stderr)
        for note in missing:
            print(note, "->", json.dumps(by_note.get(note.split(" (")[0], {}).get("recv")), file=sys.stderr)
        return 1
    path = Path(__file__).resolve().parent / "reference_only" / "act.json"
    path.write_text(json.dumps(a, indent=1, ensure_ascii=True) + "\n")
    lines = sum(1 for st in a["steps"] if st["op"] == "line")
    print(f"act: {len(a['steps'])} steps, {lines} of them lines -> {path.relative_to(REPO)}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
