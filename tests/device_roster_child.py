"""The device work of tests/test_device_roster.py, in a short-lived child process of its own.

As tests/device_many_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_ROSTER {...}``).  Every call to a ``device.Roster`` is compared with the CPU restatement
(``Cpu`` / ``expected`` / ``compare`` of tests/device_many_child.py) over listener records built from a model of the
roster kept here, slot by slot, and with ``device.broadcast_many`` over the roster's own ``table()``.

    python tests/device_roster_child.py [--seed S]
"""
from __future__ import annotations

import argparse
import json
import random
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from device_fanout_child import fuzz_items  # noqa: E402
from device_many_child import COMS, Cpu, compare, expected  # noqa: E402
from nuts333_amd import devpath, device  # noqa: E402

CAPACITIES = (1, 2, 255, 256, 257, 1000, 1015, 4096)
KS = (1, 7, 100, 1000)
ROOMS = (0, 1, 2, None)
FLAGS = ("login", "ignall", "ignshout", "colour")
ITEMS_PER_CALL = 200_000      # K is trimmed so that a call has at most about this many items
ARENA_BUDGET = 256 << 20      # and an arena bound of at most this, well under MANY_ARENA_CAP


class Model:
    """What the roster should hold, slot by slot, updated one write at a time (so the last write wins)."""

    def __init__(self, capacity: int):
        self.room = np.full(capacity, -1, dtype=np.int64)
        self.flags = {f: np.zeros(capacity, dtype=np.int64) for f in FLAGS}

    def update(self, slots, fields: dict) -> None:
        for i, s in enumerate(slots):
            for f, v in fields.items():
                v = v[i] if isinstance(v, list) else v
                if f == "room":
                    self.room[s] = -1 if v is None else v
                else:
                    self.flags[f][s] = v

    def records(self, rm, sender) -> np.ndarray:
        """Listener records (bit k = LISTENER_FIELDS[k]) of broadcast (rm, sender), by write_room_except's rules."""
        bit = {f: 1 << device.LISTENER_FIELDS.index(f) for f in device.LISTENER_FIELDS}
        out = sum(self.flags[f] * bit[f] for f in FLAGS)
        out = out | np.where(self.room >= 0, bit["has_room"], 0)
        if rm is not None:
            out = out | np.where(self.room == rm, bit["same_room"], 0)
        if sender is not None:
            out[sender] |= bit["is_sender"]
        return out

    def rooms(self) -> int:
        return int((self.room >= 0).sum())


def random_update(rng: random.Random, cap: int, roster: device.Roster, model: Model) -> None:
    """A batch of slots (repeats likely) and a random subset of the fields, each a value or one per slot."""
    slots = [rng.randrange(cap) for _ in range(rng.randint(1, max(1, cap // 3)))]
    fields = {}
    for f in ("room",) + FLAGS:
        if rng.random() < 0.6:
            pick = (lambda: rng.choice(ROOMS)) if f == "room" else (lambda: rng.randrange(2))
            fields[f] = pick() if rng.random() < 0.3 else [pick() for _ in slots]
    roster.update(slots, **fields)
    model.update(slots, fields)


def random_part(cpu: Cpu, seed: int) -> dict:
    rng = random.Random(seed)
    pool = [t for t, _ in fuzz_items(seed, 4000)]
    res = {"capacities": [], "ks": [], "calls": 0, "items": 0, "updates": 0, "calls_without_update": 0,
           "n_bad_cpu": 0, "first_bad_cpu": [], "n_bad_tables": 0, "first_bad_tables": [],
           "rm_forms": set(), "sender_forms": set()}
    seen = np.zeros(128, dtype=bool)
    for cap in CAPACITIES:
        with device.Roster(cap) as roster:
            model = Model(cap)
            for k in KS:
                if rng.random() < 0.75:
                    for _ in range(rng.randint(1, 3)):
                        random_update(rng, cap, roster, model)
                        res["updates"] += 1
                else:
                    res["calls_without_update"] += 1
                k = max(1, min(k, ITEMS_PER_CALL // cap))
                calls = [(rng.choice(pool), rng.choice(ROOMS), rng.choice([None, rng.randrange(cap)]),
                          rng.randrange(2), rng.choice(COMS)) for _ in range(k)]
                while len(calls) > 1 and model.rooms() * sum(device.max_bytes(len(c[0])) for c in calls) > ARENA_BUDGET:
                    calls = calls[:len(calls) // 2]
                r = roster.broadcast_many(calls)
                records = [model.records(rm, s) for _, rm, s, _, _ in calls]
                as_tables = [(t, roster.table(rm, s), int(rm is None), fl, com) for t, rm, s, fl, com in calls]
                bad, first = compare(r, expected(cpu, as_tables, records), as_tables)
                res["n_bad_cpu"] += bad
                res["first_bad_cpu"] += first[:5 - len(res["first_bad_cpu"])]
                same = device.broadcast_many(as_tables)
                fields = ("admitted", "out_offsets", "arena", "write_offsets", "write_sizes", "broadcast_offsets")
                if not all(np.array_equal(getattr(r, f), getattr(same, f)) for f in fields):
                    res["n_bad_tables"] += 1
                    if len(res["first_bad_tables"]) < 5:
                        res["first_bad_tables"].append({"capacity": cap, "k": len(calls)})
                for rec in records:
                    seen[rec] = True
                res["rm_forms"] |= {"every room" if c[1] is None else "room" for c in calls}
                res["sender_forms"] |= {"none" if c[2] is None else "slot" for c in calls}
                res["capacities"].append(cap)
                res["ks"].append(k)
                res["calls"] += 1
                res["items"] += len(r.admitted)
    res["records_seen"] = int(seen.sum())
    res["rm_forms"], res["sender_forms"] = sorted(res["rm_forms"]), sorted(res["sender_forms"])
    return res


def item_views(r: device.Fanout) -> list:
    return [(bool(r.admitted[i]), r.output(i), r.write_sizes[r.write_offsets[i]:r.write_offsets[i + 1]].tolist())
            for i in range(len(r.admitted))]


def updates_part(cpu: Cpu) -> list:
    """Three one-slot changes, each between two identical calls: only that slot's items may change, and the result
    returned before the change must stay as it was."""
    cap, out = 300, []
    with device.Roster(cap) as roster:
        model = Model(cap)
        roster.update(range(cap), room=0, colour=[j % 2 for j in range(cap)])
        model.update(range(cap), {"room": 0, "colour": [j % 2 for j in range(cap)]})
        calls = [(t, 0, 0, 0, device.COM_SHOUT) for t in devpath.line_texts("shout", 3)]
        for field, slot, value in (("colour", 10, 1), ("room", 7, 1), ("ignshout", 9, 1)):
            before = roster.broadcast_many(calls)
            saved = item_views(before)
            roster.update([slot], **{field: value})
            model.update([slot], {field: value})
            after = roster.broadcast_many(calls)
            records = [model.records(rm, s) for _, rm, s, _, _ in calls]
            as_tables = [(t, None, 0, fl, com) for t, rm, s, fl, com in calls]
            bad, _ = compare(after, expected(cpu, as_tables, records), as_tables)
            a, b = item_views(before), item_views(after)
            changed = sorted({i % cap for i in range(len(a)) if a[i] != b[i]})
            out.append({"field": field, "slot": slot, "changed_slots": changed, "n_bad": bad,
                        "earlier_result_unchanged": item_views(before) == saved})
    return out


def h2d_part() -> dict:
    """h2d_bytes of the first call (the table goes up), a call with nothing changed, a call after an update and one
    more with nothing changed, at capacities 256 and 4096 with the same texts."""
    out = {"dirty": {}, "clean": {}, "after_update": {}, "clean_again": {}}
    calls = [(t, 0, 0, 0, device.COM_SAY) for t in devpath.line_texts("say", 10)]
    for cap in (256, 4096):
        with device.Roster(cap) as roster:
            roster.update(range(cap), room=0)
            out["dirty"][cap] = roster.broadcast_many(calls).timing["h2d_bytes"]
            out["clean"][cap] = roster.broadcast_many(calls).timing["h2d_bytes"]
            roster.update([5], colour=1)
            out["after_update"][cap] = roster.broadcast_many(calls).timing["h2d_bytes"]
            out["clean_again"][cap] = roster.broadcast_many(calls).timing["h2d_bytes"]
    return out


def isolation_part(cpu: Cpu) -> dict:
    """Two rosters interleaved A, B, A, with broadcast() and broadcast_many() calls between, then B again."""
    fields = ("admitted", "out_offsets", "arena", "write_offsets", "write_sizes", "broadcast_offsets")
    same = lambda x, y: all(np.array_equal(getattr(x, f), getattr(y, f)) for f in fields)
    with device.Roster(300) as a, device.Roster(500) as b:
        ma, mb = Model(300), Model(500)
        a.update(range(300), room=[j % 3 for j in range(300)], colour=1)
        ma.update(range(300), {"room": [j % 3 for j in range(300)], "colour": 1})
        b.update(range(0, 500, 2), room=1, ignshout=1)
        mb.update(range(0, 500, 2), {"room": 1, "ignshout": 1})
        ca = [(t, 1, 4, 0, device.COM_SAY) for t in devpath.line_texts("say", 5)]
        cb = [(t, None, None, 1, device.COM_SHOUT) for t in devpath.line_texts("shout", 4)] + \
             [(b"~FRred\n", 1, None, 0, device.COM_SAY)]
        ra1 = a.broadcast_many(ca)
        rb1 = b.broadcast_many(cb)
        ra2 = a.broadcast_many(ca)
        tab = devpath.listeners(200, "half")
        device.broadcast(b"between\n", tab, 0, 0, device.COM_SAY)
        device.broadcast_many([(b"~OLmany\n", tab, 1, 0, device.COM_SHOUT)] * 3)
        ra3 = a.broadcast_many(ca)
        rb2 = b.broadcast_many(cb)
        bad = 0
        for r, m, calls in ((ra1, ma, ca), (rb1, mb, cb)):
            as_tables = [(t, None, int(rm is None), fl, com) for t, rm, s, fl, com in calls]
            bad += compare(r, expected(cpu, as_tables, [m.records(rm, s) for _, rm, s, _, _ in calls]), as_tables)[0]
        return {"a_repeat_identical": same(ra1, ra2) and same(ra1, ra3), "b_repeat_identical": same(rb1, rb2),
                "a_differs_from_b": ra1.arena.tobytes() != rb1.arena.tobytes(), "n_bad": bad}


def bench_step(cpu: Cpu) -> dict:
    """The bench headline's step (device_many_child.bench_step) to a roster: 100 distinct .shout lines to 1000 slots in
    room 0, slot 0 the sender, colour on every other slot."""
    tab = devpath.listeners(1000, "half")
    with device.Roster(1000) as roster:
        roster.update(range(1000), room=0, colour=tab[:, device.LISTENER_FIELDS.index("colour")])
        calls = [(t, 0, 0, 0, device.COM_SHOUT) for t in devpath.line_texts("shout", 100)]
        r = roster.broadcast_many(calls)
    as_tables = [(t, tab, 0, 0, device.COM_SHOUT) for t, _, _, _, _ in calls]
    rec = (tab.astype(np.int64) << np.arange(len(device.LISTENER_FIELDS))).sum(axis=1)
    bad, first = compare(r, expected(cpu, as_tables, [rec] * len(calls)), as_tables)
    return {"broadcasts": len(calls), "deliveries": int(r.admitted.sum()), "bytes": int(r.out_offsets[-1]),
            "n_bad": bad, "first_bad": first, "timing": r.timing}


def worst(cpu: Cpu) -> dict:
    """64 broadcasts of 1999 newlines to 64 slots with colour on, then a small call, then the large one again."""
    text = b"\n" * 1999
    with device.Roster(64) as roster:
        roster.update(range(64), room=0, colour=1)
        large = [(text, 0, None, 0, device.COM_SAY)] * 64
        a = roster.broadcast_many(large)
        roster.broadcast_many([(b"hi\n", 0, None, 0, device.COM_SAY)])
        b = roster.broadcast_many(large)
    rec = np.full(64, 2 | 4 | 64, dtype=np.int64)                        # has_room, same_room, colour
    as_tables = [(text, None, 0, 0, device.COM_SAY)] * 64
    bad, first = compare(a, expected(cpu, as_tables, [rec] * 64), as_tables)
    same = all(np.array_equal(getattr(a, f), getattr(b, f))
               for f in ("admitted", "out_offsets", "arena", "write_offsets", "write_sizes", "broadcast_offsets"))
    return {"items": len(a.admitted), "per_item": sorted({(int(x), int(y)) for x, y in
                                                           zip(np.diff(a.out_offsets), np.diff(a.write_offsets))}),
            "n_bad": bad, "first_bad": first, "reuse_identical": same}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1401)
    a = ap.parse_args()
    out = {"device_count": device.device_count()}
    if out["device_count"] < 1:
        print("device_roster_child: no GPU visible", file=sys.stderr)
        return 2
    cpu = Cpu()
    out["random"] = random_part(cpu, a.seed)
    out["updates"] = updates_part(cpu)
    out["h2d"] = h2d_part()
    out["isolation"] = isolation_part(cpu)
    out["bench_step"] = bench_step(cpu)
    out["worst"] = worst(cpu)
    print("DEVICE_ROSTER " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
