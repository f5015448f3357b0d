"""What the children of the event calls -- ``go_many``, ``access_many``, ``clone_many``, ``set_many`` -- share: the
comparison of a device result with the model's call, the digest of a result, and the frame of a child's ``main``.

A result of these calls is shaped alike: ``outcome[k]`` per event, some arrays of its own, and per kind of text a plan
and a text accessor, row ``r`` of ``text_sizes`` holding the sizes of kind ``r`` with -1 where the event has no such text.
``kinds`` below is that list as ``(kind, plan, text)`` rows, in the order of ``text_sizes``' rows; the model's event is a
dict with ``slot``, ``outcome``, the text of every kind (or None) and ``plans[kind]``, the admitted slots.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from nuts333_amd import device, nuts_path  # noqa: E402

GOLDEN = REPO / "tests" / "golden"


def plan_of(plan, k: int) -> dict:
    return {"admitted": np.flatnonzero(plan.admitted(k)).tolist(), "chunks": {c: plan.chunks(k, c) for c in (0, 1)}}


def event_differences(got, call: dict, kinds, deferred: int, fields, also_deferred=lambda k: False, effective=None) -> list:
    """Everything a result says against the model's call.  ``fields(k, res)`` gives the call's own fields of event ``k``
    as ``(have, want)``, compared after the outcome; ``also_deferred(k)`` is true where a deferred event holds something
    of the call's own that it must not; ``effective`` is the outcomes ``got.effective()`` lists, or None for a result
    without one."""
    bad = []
    for k, res in enumerate(call["events"]):
        where = {"event": k, "slot": res["slot"], **({"com": res["com"]} if "com" in res else {}), "model": res["outcome"]}
        if res["outcome"] == deferred:                                  # what it resolved to is the snapshot's: not compared
            if int(got.outcome[k]) != deferred or also_deferred(k) or (got.text_sizes[:, k] != -1).any() or any(
                    p.admitted(k).any() or p.variant_sizes[k].any() or p.write_counts[k].any() for _, p, _ in kinds):
                bad.append({**where, "what": "a deferred event", "device": int(got.outcome[k])})
            continue
        have, want = fields(k, res)
        have, want = [int(got.outcome[k]), *have], [res["outcome"], *want]
        if have != want:
            bad.append({**where, "what": "outcome", "device": have, "want": want})
            continue
        for row, (kind, plan, text) in enumerate(kinds):
            want = res[kind]
            if text(k) != (want or b"") or (got.text_sizes[row, k] >= 0) != (want is not None):
                bad.append({**where, "what": kind + " text", "device": text(k).decode("latin-1"), "want": repr(want)})
                continue
            p = plan_of(plan, k)
            want_chunks = {c: nuts_path.chunks(want, c) if want is not None else [] for c in (0, 1)}
            if p["admitted"] != res["plans"][kind] or p["chunks"] != want_chunks:
                bad.append({**where, "what": kind + " plan", "device": p["admitted"][:20], "want": res["plans"][kind][:20]})
    if effective is not None and got.effective().tolist() != [k for k, r in enumerate(call["events"]) if r["outcome"] in effective]:
        bad.append({"what": "effective", "device": got.effective().tolist()})
    return bad


def digest(got, arrays, kinds) -> str:
    """A hash of the outcomes, ``arrays`` (arrays or bytes), the text sizes and every kind's text, admit bitmap and chunks."""
    h = hashlib.sha256()
    for a in (got.outcome, *arrays, got.text_sizes):
        h.update(a if isinstance(a, bytes) else a.tobytes())
    for _, plan, text in kinds:
        for k in range(len(got.outcome)):
            h.update(text(k) + plan.admitted_bits[k].tobytes() + b"".join(b"|".join(plan.chunks(k, c)) for c in (0, 1)))
    return h.hexdigest()


def load(name: str) -> dict:
    return json.loads((GOLDEN / name).read_text())


def lines_of(doc: dict, names) -> int:
    """The session's lines whose first word is one of the commands ``names``, typed with its dot."""
    dotted = {"." + n for n in names}
    return sum(1 for s in doc["steps"] if s["op"] == "line" and (s["send"].split() or [""])[0] in dotted)


def child_main(tag: str, parts, profile=None, seed: int = 0) -> int:
    """A child's ``main``: ``parts(seed)`` gives the ``(name, function)`` pairs to run and time, the results go out as one
    ``tag {...}`` line, and ``--profile`` writes ``profile(res)`` -- the parts' seconds without one -- as JSON."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=seed)
    ap.add_argument("--profile", help="write the parts' seconds here, as JSON")
    args = ap.parse_args()
    if device.device_count() < 1:
        print("no GPU visible", file=sys.stderr)
        return 3
    res, seconds = {}, {}
    for name, part in parts(args.seed):
        t0 = time.perf_counter()
        res[name] = part()
        seconds[name] = round(time.perf_counter() - t0, 3)
    res["seconds"] = seconds
    print(tag + " " + json.dumps(res))
    if args.profile:
        Path(args.profile).write_text(json.dumps(profile(res) if profile else {"seconds": seconds}, indent=1) + "\n")
    return 0
