#!/usr/bin/env python3
"""Generate tests/golden/reference_only/access.json: a session about a room's door -- ``.private``, ``.public``,
``.letmein`` and ``.invite`` -- run against the REFERENCE build.

    make -C oracle ref                           # needs the reference source (never on the GPU box)
    python tests/golden/make_access_golden.py

As make_go_golden.py: one single-talker scenario of its own, registered in its own process.  The -O2 and the -O0
reference builds, and two runs of the same build, must give the same fixture; the script checks that before it writes.
The talker runs with ``min_private 2``, ``ignore_mp_level WIZ`` and ``gatecrash_level ARCH``, as every provisioned config
does, and ``max_clones 1``, over the shipped five rooms: the corridor and the lounge can be set, the drive and the hallway
are fixed public, the wizroom is fixed private.

Five accounts: Alice, a USER with colour; Bobby, a plain USER; Carol, a WIZ; Dave, an ARCH with colour, the only one who
may ``.invis`` and ``.clone``; Erica, a USER who sets ``.ignall``.  ``.clone`` is an ARCH's command, and an ARCH is above
``ignore_mp_level``, so "the clone counts" is shown by a USER who stands beside the ARCH's clone: alone she was refused,
beside the clone she is allowed, and the clone relays her line to its owner in another room.

What the session holds, for tests/test_device_access.py, each under a ``note`` of its own.  ``.private`` / ``.public``: a
USER alone refused; the WIZ alone allowed; a USER beside a clone allowed and relayed; two USERs; ``.private`` again;
``.public``; ``.public`` again; an invisible actor; a USER's ``.private wizroom`` (level too low); the ARCH's (fixed, "That
room's"); the WIZ's inside the wizroom (fixed, "This room's"); the ARCH setting and unsetting the lounge from the corridor
while a colour and a plain user stand in it; ``.public lou`` of the public lounge; ``.private nosuch``; a line said, then
``.public``, then ``.review``: empty; a user invited, then ``.public``, ``.private`` and the invited user's ``.go``: refused.
``.letmein``: alone; ``nosuch``; the own room; a room not adjoined; a public room; the private corridor asked from the
hallway by ``co`` with listeners in both rooms; the wizroom from its neighbour; an invisible asker.  ``.invite``: alone; in
a public room; nobody; oneself; someone already here; by a lower-case word that is a substring; the same user again; by
an invisible inviter; of the ``ignall`` user; of a user who holds an invitation to another room and then enters by the new
one.
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
PRIVATE, PUBLIC = "Room set to \x1b[31mPRIVATE", "Room set to \x1b[32mPUBLIC"
#: note -> what the actor's own bytes must hold (colour accounts get the escape, plain ones the bare word)
WANTED = {
    "a USER alone is refused": "You need at least 2 users/clones in a room before it can be made private.",
    "letmein alone": "Let you into where?", "invite alone": "Invite who?", "invite in a public room": "This room is currently public.",
    "the WIZ alone is allowed": "Room set to PRIVATE", "the WIZ makes it public": "Room set to PUBLIC",
    "inside the wizroom": "This room's access is fixed.", "a USER beside a clone: the clone counts": PRIVATE,
    "public again beside the clone": PUBLIC, "two USERs make the corridor private": "Room set to PRIVATE",
    "private again": "This room is already private.", "public": PUBLIC, "public again": "This room is already public.",
    "an invisible actor": PRIVATE, "level too low": "You are not a high enough level to use the room option.",
    "that room's access is fixed": "That room's access is fixed.", "the ARCH sets the lounge from the corridor": PRIVATE,
    "the ARCH unsets the lounge": PUBLIC, "that room is already public": "That room is already public.",
    "private nosuch": "There is no such room.", "public clears the review buffer": PUBLIC, "the buffer is empty": "Review buffer is empty.",
    "an invitation": "You invite Carol in.", "the invitation was cleared": "That room is currently private, you cannot enter.",
    "letmein nosuch": "There is no such room.", "letmein own room": "You are already in the drive!",
    "letmein not adjoined": "The lounge is not adjoined to here.", "letmein a public room": "The drive is currently public.",
    "the private corridor asked from the hallway": "You shout asking to be let into the corridor.",
    "the wizroom asked from its neighbour": "You shout asking to be let into the wizroom.",
    "an invisible asker": "You shout asking to be let into the wizroom.",
    "invite nobody": "There is no one of that name logged on.", "invite oneself": "Inviting yourself to somewhere is the third sign of madness.",
    "invite someone already here": "Dave is already here!", "invite by a lower-case substring": "You invite Carol in.",
    "the same user again": "Carol has already been invited into here.", "an invisible inviter": "You invite Alice in.",
    "the ignall user still receives the notice": "You invite Erica in.", "an invitation over another": "You invite Carol in.",
    "entering by the new invitation": "Access is ", "the old invitation is gone": "That room is currently private, you cannot enter.",
}
#: (note, client, needle): what somebody else must have been sent
HEARD = (
    ("a USER beside a clone: the clone counts", "d", "[ corridor ]:\x1b[0m Alice has set the room to \x1b[31mPRIVATE"),
    ("two USERs make the corridor private", "a", "Bobby has set the room to \x1b[31mPRIVATE"),
    ("an invisible actor", "b", "A presence has set the room to PRIVATE"),
    ("the ARCH sets the lounge from the corridor", "b", "This room has been set to PRIVATE"),
    ("the ARCH sets the lounge from the corridor", "a", "This room has been set to \x1b[31mPRIVATE"),
    ("an invitation", "c", "Alice has invited you into the lounge."),
    ("the private corridor asked from the hallway", "c", "Erica shouts asking to be let into the corridor."),
    ("the private corridor asked from the hallway", "b", "Erica shouts asking to be let in."),
    ("the wizroom asked from its neighbour", "c", "Erica shouts asking to be let in."),
    ("an invisible asker", "e", "Dave shouts asking to be let into the wizroom."),
    ("an invisible asker", "c", "Dave shouts asking to be let in."),
    ("an invisible inviter", "a", "A presence has invited you into the corridor."),
    ("the ignall user still receives the notice", "e", "A presence has invited you into the corridor."),
)


def access():
    accounts = [pv.Account("Alice", level=1, colour=1), pv.Account("Bobby", level=1), pv.Account("Carol", level=2),
                pv.Account("Dave", level=3, colour=1), pv.Account("Erica", level=1)]

    def configs(p):
        return [pv.TalkerConfig(mainport=p[0][0], wizport=p[0][1], linkport=p[0][2], max_users=50, max_clones=1)]

    def script(s):
        for k, a in zip("abcde", accounts):
            s.connect(k); s.login(k, a.name, colour=bool(a.colour))
        # -- .private and .public
        s.line("a", ".go hallway")
        s.line("a", ".go corridor")
        s.line("a", ".private", note="a USER alone is refused")
        s.line("a", ".letmein", note="letmein alone")
        s.line("a", ".invite", note="invite alone")
        s.line("a", ".invite bobby", note="invite in a public room")
        for room in ("hallway", "corridor", "lounge"):
            s.line("c", ".go " + room)
        s.line("c", ".private", note="the WIZ alone is allowed")
        s.line("c", ".public", note="the WIZ makes it public")
        s.line("c", ".go wizroom")
        s.line("c", ".private", note="inside the wizroom")
        s.line("d", ".clone corridor", note="a clone beside the USER")
        s.line("a", ".private", note="a USER beside a clone: the clone counts")
        s.line("a", ".public", note="public again beside the clone")
        s.line("d", ".destroy corridor")
        s.line("b", ".go hallway")
        s.line("b", ".go corridor")
        s.line("b", ".private", note="two USERs make the corridor private")
        s.line("b", ".private", note="private again")
        s.line("a", ".public", note="public")
        s.line("a", ".public", note="public again")
        s.line("d", ".invis")
        s.line("d", ".go hallway")
        s.line("d", ".go corridor")
        s.line("d", ".private", note="an invisible actor")
        s.line("b", ".private wizroom", note="level too low")
        s.line("d", ".private wizroom", note="that room's access is fixed")
        s.line("a", ".go lounge")
        s.line("b", ".go lounge", note="the ARCH alone stays behind: the corridor returns to public")
        s.line("d", ".private lounge", note="the ARCH sets the lounge from the corridor")
        s.line("d", ".public lou", note="the ARCH unsets the lounge")
        s.line("d", ".public lou", note="that room is already public")
        s.line("d", ".private nosuch", note="private nosuch")
        s.line("d", ".private lounge")
        s.line("a", "a line for the review buffer")
        s.line("a", ".public", note="public clears the review buffer")
        s.line("a", ".review", note="the buffer is empty")
        s.line("a", ".private")
        s.line("a", ".invite carol", note="an invitation")
        s.line("a", ".public")
        s.line("a", ".private")
        s.line("c", ".go lounge", note="the invitation was cleared")
        # -- .letmein
        s.line("e", ".letmein nosuch", note="letmein nosuch")
        s.line("e", ".letmein drive", note="letmein own room")
        s.line("e", ".letmein lounge", note="letmein not adjoined")
        s.line("e", ".go hallway")
        s.line("e", ".letmein dri", note="letmein a public room")
        s.line("b", ".go corridor")
        s.line("d", ".private")
        s.line("c", ".go hallway")
        s.line("e", ".letmein co", note="the private corridor asked from the hallway")
        s.line("c", ".go wizroom")
        s.line("e", ".letmein wiz", note="the wizroom asked from its neighbour")
        s.line("d", ".go hallway")
        s.line("d", ".letmein wizroom", note="an invisible asker")
        # -- .invite
        s.line("d", ".go corridor")
        s.line("d", ".private")
        s.line("b", ".invite nobody", note="invite nobody")
        s.line("b", ".invite bobby", note="invite oneself")
        s.line("b", ".invite dave", note="invite someone already here")
        s.line("b", ".invite car", note="invite by a lower-case substring")
        s.line("b", ".invite carol", note="the same user again")
        s.line("d", ".invite alice", note="an invisible inviter")
        s.line("e", ".ignall")
        s.line("d", ".invite erica", note="the ignall user still receives the notice")
        s.line("d", ".private lounge")
        s.line("a", ".invite carol", note="an invitation over another")
        s.line("c", ".go lounge", note="entering by the new invitation")
        s.line("c", ".go corridor", note="the old invitation is gone")

    return {"configs": configs, "accounts": [accounts], "boot_order": [0], "script": script, "config_kw": CONFIG}


def main() -> int:
    scenarios.REFERENCE_ONLY["access"] = access
    if not REF_BINARY.exists():
        print("oracle/_ref/nuts333 is missing: run `make -C oracle ref` first", file=sys.stderr)
        return 2
    a = run_scenario("access", REF_BINARY)
    b = run_scenario("access", REF_BINARY_O0) if REF_BINARY_O0.exists() else a
    if a != b:
        print("access: -O2 and -O0 reference builds disagree", file=sys.stderr)
        return 1
    if a != run_scenario("access", REF_BINARY):
        print("access: two runs of the same build disagree (nondeterministic capture)", file=sys.stderr)
        return 1
    by_note = {st.get("note"): st for st in a["steps"] if st.get("note")}
    missing = [note for note, needle in WANTED.items() if needle not in by_note.get(note, {"recv": {}, "actor": ""})["recv"].get(
        by_note.get(note, {"actor": ""})["actor"], "")]
    missing += [f"{note} ({client})" for note, client, needle in HEARD if needle not in by_note[note]["recv"].get(client, "")]
    if missing:
        print(f"access: steps that did not go as the session claims: {missing}", file=sys.stderr)
        return 1
    path = Path(__file__).resolve().parent / "reference_only" / "access.json"
    path.write_text(json.dumps(a, indent=1, ensure_ascii=True) + "\n")
    lines = sum(1 for st in a["steps"] if st["op"] == "line")
    print(f"access: {len(a['steps'])} steps, {lines} of them lines -> {path.relative_to(REPO)}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
