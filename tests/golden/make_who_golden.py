#!/usr/bin/env python3
"""Generate tests/golden/reference_only/who.json: a session with ``.who`` in it, run against the REFERENCE build.

    make -C oracle ref                           # needs the reference source (never on the GPU box)
    python tests/golden/make_who_golden.py

No scenario of tests/scenarios.py types ``.who``, and the restated talker does not answer it, so this script registers
one single-talker scenario of its own, in its own process, and records it as make_golden.py records the others: the
provisioning, the input lines and, per step, the bytes each client received.  who()'s header carries ``long_date(1)``
("on <Day> <d> <Month> <yyyy> at HH:MM", nuts333.c:2619), which is replaced by the literal ``DATE``.  The -O2 and the -O0
reference builds, and two runs of the same build, must give the same fixture; the script checks that before it writes.

What the session holds, for tests/test_device_who.py: five users of the levels NEW .. ARCH and a GOD in two rooms,
descriptions with ``~FR``, ``~FBK``, ``~FBBM`` (colour_com_count counts them 1, 2 and 3) and plain ones, a looker with
colour on, an ARCH who goes invisible (``.invis`` is an ARCH's command) and is then looked for from below, from above and
by itself, a user who is AFK, a ``.go`` between two whos, and ``who`` typed at the name prompt.
"""
from __future__ import annotations

import json
import re
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from nuts333_amd import provision as pv                      # noqa: E402
from nuts333_amd.talker import REF_BINARY, REF_BINARY_O0    # noqa: E402
import scenarios                                            # noqa: E402
from scenario_runner import run_scenario                    # noqa: E402

_WHO_DATE = re.compile(r"(\*\*\* Current users )on [A-Z][a-z]+ \d{1,2} [A-Z][a-z]+ \d{4} at \d\d:\d\d( \*\*\*)")


def who():
    accounts = [pv.Account("Alice", level=1, colour=1, desc="~FRis red"),
                pv.Account("Bobby", level=0, desc="~FBKcounts two"),
                pv.Account("Carol", level=2, desc="~FBBMthree and~OLItwo"),
                pv.Account("Dave", level=3, desc="is a plain arch"),
                pv.Account("Erica", level=1, desc="is erica"),
                pv.Account("Frank", level=4, desc="is a god")]

    def script(s):
        for k, a in zip("abcdef", accounts):
            s.connect(k); s.login(k, a.name, colour=bool(a.colour))
        s.line("a", ".who", note="colour on")
        s.line("b", ".who", note="colour off, level NEW")
        s.line("d", ".go hallway")
        s.line("d", ".invis")
        s.line("b", ".who", note="an invisible ARCH is hidden from below")
        s.line("c", ".who", note="... from a WIZ too")
        s.line("f", ".who", note="... shown with a * from above")
        s.line("d", ".who", note="... and to itself, at equal level")
        s.line("e", ".afk", can_sync=False)
        s.line("a", ".who", note="an AFK user")
        s.line("a", ".go hallway")
        s.line("a", ".who", note="after a .go")
        s.connect("x")
        s.dialog("x", "who", expect=b"Give me a name: ", note="at the name prompt: the plain header")

    return {}, accounts, script


def record(binary) -> dict:
    out = run_scenario("who", binary)
    for st in out["steps"]:
        st["recv"] = {k: _WHO_DATE.sub(r"\1DATE\2", v) for k, v in st["recv"].items()}
    return out


def main() -> int:
    scenarios.REFERENCE_ONLY["who"] = who
    if not REF_BINARY.exists():
        print("oracle/_ref/nuts333 is missing: run `make -C oracle ref` first", file=sys.stderr)
        return 2
    a = record(REF_BINARY)
    b = record(REF_BINARY_O0) if REF_BINARY_O0.exists() else a
    if a != b:
        print("who: -O2 and -O0 reference builds disagree", file=sys.stderr)
        return 1
    if a != record(REF_BINARY):
        print("who: two runs of the same build disagree (nondeterministic capture)", file=sys.stderr)
        return 1
    whos = sum(1 for st in a["steps"] if st.get("send") in (".who", "who"))
    if not all("Current users DATE" in st["recv"].get(st["actor"], "") for st in a["steps"] if st.get("send") in (".who", "who")):
        print("who: a who step without its header", file=sys.stderr)
        return 1
    path = Path(__file__).resolve().parent / "reference_only" / "who.json"
    path.write_text(json.dumps(a, indent=1, ensure_ascii=True) + "\n")
    print(f"who: {len(a['steps'])} steps, {whos} whos -> {path.relative_to(REPO)}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
