#!/usr/bin/env python3
"""Generate tests/golden/reference_only/rmst.json: a session with ``.rmst`` and ``.rmsn`` in it, run against the REFERENCE
build.  (tests/golden/rooms.json is another scenario, hence the name.)

    make -C oracle ref                           # needs the reference source (never on the GPU box)
    python tests/golden/make_rmst_golden.py

No scenario of tests/scenarios.py types either command, and the restated talker does not answer them, so this script
registers one single-talker scenario of its own, in its own process, and records it as make_who_golden.py records its
session.  The -O2 and the -O0 reference builds, and two runs of the same build, must give the same fixture; the script
checks that before it writes.

What the session holds, for tests/test_device_rooms.py: a USER with colour on, a NEW user, a WIZ and an ARCH in three
rooms; both listings from the colour-on and from a colour-off looker; a topic set with ``.topic`` that holds a colour
command; a one-line ``.write``, so that a ``mesg_cnt`` is 1; a room made private with ``.private`` (the corridor) beside
the FIXED rooms of the shipped config (``*~FGPUB`` and ``*~FRPRIV``); a ``.go`` between two listings; an invisible ARCH,
who is counted; a clone of his in the hallway, which is not; and a second connection sitting at the name prompt, which
is not counted either.

The netlink columns: the lounge is the shipped config's ACCEPT room, so its inlink is ``YES`` and, with no netlink, its
state ``~FRDOWN``; the corridor is given a netlink to a site nobody dials (``auto_connect`` is off), so its link is
UNCONNECTED and ``.rmsn`` prints ``~FRDOWN`` with the service name; every other room prints ``   -``.  The UP and VER
states need a second talker and stay covered by the model alone.
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

#: the service of the corridor's netlink, which is never dialled
SERVICE = "faraway"
LISTINGS = (".rmst", ".rmsn")


def rmst():
    accounts = [pv.Account("Alice", level=1, colour=1), pv.Account("Bobby", level=0), pv.Account("Carol", level=2),
                pv.Account("Dave", level=3)]

    def configs(p):
        rooms = tuple(pv.Room(r.label, r.name, r.links, r.access, f"CONNECT {SERVICE}" if r.name == "corridor" else r.netlink,
                              r.description) for r in pv.DEFAULT_ROOMS)
        return [pv.TalkerConfig(mainport=p[0][0], wizport=p[0][1], linkport=p[0][2], max_users=50, rooms=rooms,
                                sites=[pv.Site(SERVICE, "127.0.0.1", 9, "verify2")])]

    def script(s):
        for k, a in zip("abcd", accounts):
            s.connect(k); s.login(k, a.name, colour=bool(a.colour))
        s.line("a", ".rmst", note="colour on")
        s.line("b", ".rmst", note="colour off")
        s.line("a", ".rmsn", note="colour on")
        s.line("b", ".rmsn", note="colour off")
        s.line("a", ".topic a ~FGgreen~RS topic")
        s.line("a", ".write one line on the board")
        for hop in pv.WALKS["corridor"]:
            s.line("c", f".go {hop}")
        s.line("c", ".private")
        s.line("d", ".clone hallway")
        s.line("d", ".invis")
        s.connect("x")
        s.line("b", ".rmst", note="a topic, a message, a private room; the clone and the name prompt are not counted")
        s.line("a", ".rmsn", note="the invisible user is counted")
        s.line("a", ".go hallway", note="where the clone stands (.go is a USER's command)")
        s.line("b", ".rmst", note="after a .go")
        s.line("a", ".rmst", note="after a .go, colour on")
        s.line("b", ".rmsn", note="after a .go")

    return {"configs": configs, "accounts": [accounts], "boot_order": [0], "script": script}


def main() -> int:
    scenarios.REFERENCE_ONLY["rmst"] = rmst
    if not REF_BINARY.exists():
        print("oracle/_ref/nuts333 is missing: run `make -C oracle ref` first", file=sys.stderr)
        return 2
    a = run_scenario("rmst", REF_BINARY)
    b = run_scenario("rmst", REF_BINARY_O0) if REF_BINARY_O0.exists() else a
    if a != b:
        print("rmst: -O2 and -O0 reference builds disagree", file=sys.stderr)
        return 1
    if a != run_scenario("rmst", REF_BINARY):
        print("rmst: two runs of the same build disagree (nondeterministic capture)", file=sys.stderr)
        return 1
    listings = [st for st in a["steps"] if st.get("send") in LISTINGS]
    if not all("*** Rooms data ***" in st["recv"].get(st["actor"], "") for st in listings):
        print("rmst: a listing step without its header", file=sys.stderr)
        return 1
    path = Path(__file__).resolve().parent / "reference_only" / "rmst.json"
    path.write_text(json.dumps(a, indent=1, ensure_ascii=True) + "\n")
    print(f"rmst: {len(a['steps'])} steps, {len(listings)} listings -> {path.relative_to(REPO)}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
