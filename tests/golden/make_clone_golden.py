#!/usr/bin/env python3
"""Generate tests/golden/reference_only/clone.json: a session about the clone commands -- ``.clone``, ``.destroy``,
``.csay`` and ``.chear`` -- run against the REFERENCE build.

    make -C oracle ref                           # needs the reference source (never on the GPU box)
    python tests/golden/make_clone_golden.py

As make_access_golden.py: one single-talker scenario of its own, registered in its own process.  The -O2 and the -O0
reference builds, and two runs of the same build, must give the same fixture; the script checks that before it writes.
The talker runs with ``max_clones 2``, so that "already have one there" and "maximum reached" are both reached with two
clones in the list, with ``ban_swearing YES``, which a ``.csay`` is not held to, with ``min_private 2`` and ``ignore_mp_level
WIZ`` as every provisioned config, and with ``gatecrash_level GOD``: ``.clone`` is an ARCH's command, and at the usual
``gatecrash_level ARCH`` no ARCH is ever refused a private room.  Over the shipped five rooms: the corridor and the lounge
can be set, the drive and the hallway are fixed public, the wizroom is fixed private.

Five accounts: Alice, a USER with colour, and Bobby, a plain USER, who listen; Dave, an ARCH with colour, invisible for a
part of the session; Eddie, a plain ARCH; Gail, a GOD, who destroys another's clone and muzzles an ARCH.

What the session holds, for tests/test_device_clone.py, each under a ``note`` of its own.  ``.clone``: here; here again; in
another room; a third one; in the room of the second of two; nowhere; after a ``.destroy`` with the actor standing beside its
clone, by a room prefix; in a private room without and with an invitation; in the wizroom; by an invisible actor.
``.destroy``: a room returned to public, with a line said before it and ``.review`` after it: empty; a room left private
because enough remain; the GOD's, with the owner notified, by a lower-case name; the same again; nobody; a higher level;
no such room; no clone there; by an invisible actor.  ``.csay``: ending in neither ``?`` nor ``!``, in ``?`` and in ``!``,
heard by two users and by a second clone in the room; a swear word; alone; a room alone; no such room; no clone there; by a
muzzled owner.  ``.chear``: the three words; a mis-cased one; a room alone; no such room; no clone there.
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

CONFIG = {"max_clones": 2, "ban_swearing": True, "min_private": 2, "ignore_mp_level": 2, "gatecrash_level": 4}
CREATED, DESTROYED = "You whisper a haunting spell and a clone is created ", "You whisper a sharp spell and the clone is destroyed."
NO_CLONE = "You do not have a clone in that room."
#: note -> what the actor's own bytes must hold
WANTED = {
    "a clone created here": CREATED + "here.", "already one here": "You already have a clone in the drive.",
    "a clone created elsewhere": CREATED + "in the lounge.", "the maximum": "You already have the maximum number of clones allowed.",
    "already one there, behind another": "You already have a clone in the lounge.", "clone nosuch": "There is no such room.",
    "destroy beside the clone": DESTROYED + "\x1b[0m\n\r\x1b[0m\x1b[35m\x1b[1mThe clone of Dave shimmers and vanishes.",
    "created by a room prefix": CREATED + "in the hallway.",
    "a private room without an invitation": "That room is currently private, you cannot create a clone there.",
    "a private room with an invitation": CREATED + "in the corridor.", "one in the wizroom": CREATED + "in the wizroom.",
    "a destroy returns the room to public": DESTROYED, "the buffer is empty": "Review buffer is empty.",
    "a destroy leaves the room private": DESTROYED, "the room is still private": "This room is already private.",
    "the GOD destroys another's clone": DESTROYED, "the same again": "Eddie does not have a clone the wizroom.",
    "destroy nobody's": "There is no one of that name logged on.",
    "a higher level": "You cannot destroy the clone of a user of an equal or higher level.", "destroy nosuch": "There is no such room.",
    "no clone there": "You do not have a clone in the corridor.",
    "csay": "[ lounge ]:\x1b[0m Clone of Dave says: hello there", "csay asks": "Clone of Dave asks: what is this?",
    "csay exclaims": "Clone of Dave exclaims: look out!", "csay swears": "Clone of Dave says: oh shit",
    "a say swears": "Swearing is not allowed here.", "csay alone": "Usage: csay <room clone is in> <message>",
    "csay a room alone": "Usage: csay <room clone is in> <message>", "csay nosuch": "There is no such room.", "csay no clone": NO_CLONE,
    "a muzzled owner": "You are muzzled, your clone cannot speak.",
    "chear swears": "Clone will now only hear swearing.", "chear nothing": "Clone will now hear nothing.",
    "chear all": "Clone will now hear everything.", "chear a mis-cased word": "Usage: chear <room clone is in> all/swears/nothing",
    "chear a room alone": "Usage: chear <room clone is in> all/swears/nothing", "chear nosuch": "There is no such room.",
    "chear no clone": NO_CLONE, "an invisible destroyer": DESTROYED, "an invisible creator": CREATED + "in the hallway.",
}
#: (note, client, needle): what somebody else must have been sent
HEARD = (
    ("a clone created here", "a", "Dave whispers a haunting spell..."),
    ("a clone created here", "b", "A clone of Dave appears in a swirling magical mist!"),
    ("a clone created elsewhere", "b", "Dave whispers a haunting spell..."),
    ("destroy beside the clone", "a", "Dave whispers a sharp spell..."),
    ("destroy beside the clone", "b", "The clone of Dave shimmers and vanishes."),
    ("a private room with an invitation", "a", "A clone of Eddie appears in a swirling magical mist!"),
    ("a destroy returns the room to public", "b", "Room access returned to PUBLIC."),
    ("a destroy returns the room to public", "b", "The clone of Eddie shimmers and vanishes."),
    ("a destroy leaves the room private", "a", "The clone of Eddie shimmers and vanishes."),
    ("the GOD destroys another's clone", "e", "Gail has destroyed your clone in the wizroom."),
    ("csay", "a", "Clone of Dave says: hello there"), ("csay", "b", "Clone of Dave says: hello there"),
    ("csay", "e", "[ lounge ]: Clone of Dave says: hello there"),
    ("csay swears", "b", "Clone of Dave says: oh shit"),
    ("an invisible destroyer", "g", "A presence whispers a sharp spell..."),
    ("an invisible creator", "g", "A presence whispers a haunting spell..."),
    ("an invisible creator", "b", "A clone of Dave appears in a swirling magical mist!"),
)
#: (note, client, needle): what somebody must not have been sent
UNHEARD = (("a destroy leaves the room private", "a", "Room access returned"), ("chear nothing, then a line", "d", "[ lounge ]"))


class Config(pv.TalkerConfig):
    """The provisioned config with ``gatecrash_level GOD``."""

    def render(self) -> str:
        text = super().render()
        assert text.count("gatecrash_level    ARCH") == 1
        return text.replace("gatecrash_level    ARCH", "gatecrash_level    GOD")


def clone():
    accounts = [pv.Account("Alice", level=1, colour=1), pv.Account("Bobby", level=1), pv.Account("Dave", level=3, colour=1),
                pv.Account("Eddie", level=3), pv.Account("Gail", level=4)]

    def configs(p):
        return [Config(mainport=p[0][0], wizport=p[0][1], linkport=p[0][2], max_users=50, max_clones=2, ban_swearing=True)]

    def script(s):
        for k, a in zip("abdeg", accounts):
            s.connect(k); s.login(k, a.name, colour=bool(a.colour))
        # -- .clone, and a .destroy beside the clone
        s.line("d", ".clone", note="a clone created here")
        s.line("d", ".clone", note="already one here")
        s.line("d", ".clone lounge", note="a clone created elsewhere")
        s.line("d", ".clone corridor", note="the maximum")
        s.line("d", ".clone lounge", note="already one there, behind another")
        s.line("d", ".clone nosuch", note="clone nosuch")
        s.line("d", ".destroy", note="destroy beside the clone")
        s.line("d", ".clone hall", note="created by a room prefix")
        # -- a private room, and the wizroom
        for k in "ab":
            s.line(k, ".go hallway")
            s.line(k, ".go corridor")
        s.line("b", ".private")
        s.line("e", ".clone corridor", note="a private room without an invitation")
        s.line("a", ".invite eddie")
        s.line("e", ".clone corridor", note="a private room with an invitation")
        s.line("e", ".clone wizroom", note="one in the wizroom")
        # -- .destroy and reset_access
        s.line("a", ".go lounge")
        s.line("b", "a line for the review buffer")
        s.line("e", ".destroy corridor", note="a destroy returns the room to public")
        s.line("b", ".review", note="the buffer is empty")
        s.line("a", ".go corridor")
        s.line("a", ".private")
        s.line("a", ".invite eddie")
        s.line("e", ".clone corridor")
        s.line("e", ".destroy corridor", note="a destroy leaves the room private")
        s.line("a", ".private", note="the room is still private")
        s.line("g", ".destroy wizroom eddie", note="the GOD destroys another's clone")
        s.line("g", ".destroy wizroom eddie", note="the same again")
        s.line("g", ".destroy wizroom nobody", note="destroy nobody's")
        s.line("e", ".destroy drive gail", note="a higher level")
        s.line("d", ".destroy nosuch", note="destroy nosuch")
        s.line("d", ".destroy corridor", note="no clone there")
        # -- .csay: Dave's clone in the lounge, two users and Eddie's clone beside it
        s.line("a", ".public")
        for k in "ab":
            s.line(k, ".go lounge")
        s.line("e", ".clone lounge")
        s.line("d", ".csay lounge hello there", note="csay")
        s.line("d", ".csay lounge what is this?", note="csay asks")
        s.line("d", ".csay lounge look out!", note="csay exclaims")
        s.line("d", ".csay lounge oh shit", note="csay swears")
        s.line("d", "oh shit", note="a say swears")
        s.line("d", ".csay", note="csay alone")
        s.line("d", ".csay lounge", note="csay a room alone")
        s.line("d", ".csay nosuch hello", note="csay nosuch")
        s.line("d", ".csay corridor hello", note="csay no clone")
        s.line("g", ".muzzle eddie")
        s.line("e", ".csay lounge hello", note="a muzzled owner")
        s.line("g", ".unmuzzle eddie")
        # -- .chear
        s.line("d", ".chear lounge swears", note="chear swears")
        s.line("a", "a clean line")
        s.line("d", ".chear lounge nothing", note="chear nothing")
        s.line("b", "a line nobody relays to Dave", note="chear nothing, then a line")
        s.line("d", ".chear lounge all", note="chear all")
        s.line("d", ".chear lounge All", note="chear a mis-cased word")
        s.line("d", ".chear lounge", note="chear a room alone")
        s.line("d", ".chear nosuch all", note="chear nosuch")
        s.line("d", ".chear corridor all", note="chear no clone")
        # -- an invisible ARCH
        s.line("b", ".go corridor")
        s.line("b", ".go hallway")
        s.line("d", ".invis")
        s.line("d", ".destroy hall", note="an invisible destroyer")
        s.line("d", ".clone hall", note="an invisible creator")
        s.line("d", ".vis")

    return {"configs": configs, "accounts": [accounts], "boot_order": [0], "script": script, "config_kw": CONFIG}


def main() -> int:
    scenarios.REFERENCE_ONLY["clone"] = clone
    if not REF_BINARY.exists():
        print("oracle/_ref/nuts333 is missing: run `make -C oracle ref` first", file=sys.stderr)
        return 2
    a = run_scenario("clone", REF_BINARY)
    b = run_scenario("clone", REF_BINARY_O0) if REF_BINARY_O0.exists() else a
    if a != b:
        print("clone: -O2 and -O0 reference builds disagree", file=sys.stderr)
        return 1
    if a != run_scenario("clone", REF_BINARY):
        print("clone: two runs of the same build disagree (nondeterministic capture)", file=sys.stderr)
        return 1
    by_note = {st.get("note"): st for st in a["steps"] if st.get("note")}
    missing = [note for note, needle in WANTED.items() if needle not in by_note.get(note, {"recv": {}, "actor": ""})["recv"].get(
        by_note.get(note, {"actor": ""})["actor"], "")]
    missing += [f"{note} ({client})" for note, client, needle in HEARD if needle not in by_note[note]["recv"].get(client, "")]
    missing += [f"{note} ({client}, not)" for note, client, needle in UNHEARD if needle in by_note[note]["recv"].get(client, "")]
    if missing:
        print(f"clone: steps that did not go as the session claims: {missing}", file=sys.stderr)
        for note in missing:
            st = by_note.get(note.split(" (")[0])
            print(note, "->", st and st["recv"], file=sys.stderr)
        return 1
    path = Path(__file__).resolve().parent / "reference_only" / "clone.json"
    path.write_text(json.dumps(a, indent=1, ensure_ascii=True) + "\n")
    lines = sum(1 for st in a["steps"] if st["op"] == "line")
    print(f"clone: {len(a['steps'])} steps, {lines} of them lines -> {path.relative_to(REPO)}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
