"""The device work of tests/test_device_replay.py, in a short-lived child process of its own.

As tests/device_who_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON line
it prints (``DEVICE_REPLAY {...}``).  Every session of tests/golden/reference_only/replay_*.json is replayed by
tests/session_replay.py through ``DeviceBackend`` -- one ``Roster`` per session, seated at the logins and left to keep its own
state after them -- twice: with the users seated next to each other in an 8-slot roster, and with the users seated at slots 0, 63, 64, 255, 256
and between them in a 257-slot one.  (Both rosters have one more slot per possible clone behind those: look() lists the
clones.)  The result holds, per session and layout, the counts of answered steps, client comparisons, comparisons of the
roster's mirrors with the replayer's state and plan comparisons between ``relay_many`` and the call that composed a line, the
Roster calls made, the ``update`` / ``set_clones`` / ``set_rooms`` calls the backend made after the logins by what they
addressed, and every mismatch -- a mirror that differs is one.

    python tests/device_replay_child.py [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from nuts333_amd import device  # noqa: E402
from session_replay import COMPACT, SEEDS, SPREAD, DeviceBackend, load, replay  # noqa: E402

KEPT = ("answered", "tracked", "comparisons", "plan_checks", "plan_disagreements", "capacity", "slots", "calls", "commands",
        "mirror_checks", "uploads")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the result, as JSON, to this file")
    a = ap.parse_args()
    out = {"device_count": device.device_count(), "sessions": {}}
    if out["device_count"] < 1:
        print("device_replay_child: no GPU visible", file=sys.stderr)
        return 2
    t0 = time.monotonic()
    for seed in SEEDS:
        doc = load(seed)
        for layout in (COMPACT, SPREAD):
            res = replay(doc, DeviceBackend, layout)
            out["sessions"][f"{seed}/{layout}"] = {**{k: res[k] for k in KEPT}, "n_mismatches": len(res["mismatches"]),
                                                   "mismatches": res["mismatches"][:3]}
    out["wall_s"] = round(time.monotonic() - t0, 2)
    out["steps"] = sum(s["answered"] + s["tracked"] for s in out["sessions"].values())
    out["device_calls"] = sum(sum(s["calls"].values()) for s in out["sessions"].values())
    text = json.dumps(out)
    if a.out:
        Path(a.out).write_text(text + "\n")
    print("DEVICE_REPLAY " + text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
