"""The device work of tests/test_device_plan.py, in a short-lived child process of its own.

As tests/device_roster_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_PLAN {...}``).  Every ``Roster.plan_many`` call is compared at plan level with the CPU
restatement (``Cpu`` of tests/device_many_child.py over the records of a ``Model`` of the roster kept here: admit bits,
both variants' bytes and chunk sizes, the tail bits, the colour bits), and its ``expand()`` with
``Roster.broadcast_many`` of the same call on the same roster.

    python tests/device_plan_child.py [--seed S] [--model-only]

``--model-only`` walks the random sequence with the model alone, no device, and prints its coverage.
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
from device_roster_child import ARENA_BUDGET, CAPACITIES, ITEMS_PER_CALL, KS, ROOMS, Model, random_update  # noqa: E402
from nuts333_amd import devpath, device  # noqa: E402

FIELDS = ("admitted", "out_offsets", "arena", "write_offsets", "write_sizes", "broadcast_offsets")
PLAN_ARRAYS = ("admitted_bits", "colour_bits", "variants", "variant_starts", "variant_sizes", "write_counts",
               "write_sizes")


def same(x: device.Fanout, y: device.Fanout) -> bool:
    return all(np.array_equal(getattr(x, f), getattr(y, f)) for f in FIELDS)


def pack(flags: np.ndarray) -> np.ndarray:
    """bool [capacity] -> uint64 [W], slot j at bit j % 64 of word j // 64, the tail bits zero."""
    padded = np.zeros((len(flags) + 63) // 64 * 64, dtype=bool)
    padded[:len(flags)] = flags
    return np.packbits(padded, bitorder="little").view(np.uint64)


def plan_differences(cpu: Cpu, plan: device.Plan, calls, model: Model) -> list:
    """What of ``plan`` differs from the restatement: one entry per broadcast and kind of difference."""
    bad = []
    cap = plan.capacity
    words = (cap + 63) // 64
    if plan.admitted_bits.shape != (len(calls), words) or plan.admitted_bits.dtype != np.uint64:
        return [{"what": "shape of admitted_bits", "got": list(plan.admitted_bits.shape)}]
    if not np.array_equal(plan.colour_bits, pack(model.flags["colour"] != 0)):
        bad.append({"what": "colour_bits"})
    for b, (text, rm, sender, force_listen, com) in enumerate(calls):
        want = cpu.admit(int(rm is None), force_listen, com)[model.records(rm, sender)]
        if not np.array_equal(plan.admitted_bits[b], pack(want)):      # the tail bits of the last word included
            bad.append({"what": "admit bits", "broadcast": b, "capacity": cap})
        if not np.array_equal(plan.admitted(b), want):
            bad.append({"what": "admitted()", "broadcast": b, "capacity": cap})
        for c in (0, 1):
            ch = cpu.chunks(text, c)
            n = int(plan.write_counts[b, c])
            if (plan.variant(b, c) != b"".join(ch) or n != len(ch)
                    or plan.write_sizes[b, c, :n].tolist() != [len(x) for x in ch]):
                bad.append({"what": "variant", "broadcast": b, "colour": c, "len": len(text),
                            "text": text[:120].decode("latin-1"), "device_bytes": int(plan.variant_sizes[b, c]),
                            "cpu_bytes": sum(map(len, ch)), "device_writes": n, "cpu_writes": len(ch)})
    return bad


def random_part(cpu: Cpu, seed: int, model_only: bool = False) -> dict:
    """The seeded sequence of device_roster_child.random_part, each call made through plan_many."""
    rng = random.Random(seed)
    pool = [t for t, _ in fuzz_items(seed, 4000)]
    res = {"capacities": [], "ks": [], "calls": 0, "items": 0, "updates": 0, "calls_without_update": 0,
           "n_bad_plan": 0, "first_bad_plan": [], "n_bad_expand": 0, "first_bad_expand": [],
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
                if not model_only:
                    plan = roster.plan_many(calls)
                    bad = plan_differences(cpu, plan, calls, model)
                    res["n_bad_plan"] += len(bad)
                    res["first_bad_plan"] += bad[:5 - len(res["first_bad_plan"])]
                    if not same(plan.expand(), roster.broadcast_many(calls)):
                        res["n_bad_expand"] += 1
                        if len(res["first_bad_expand"]) < 5:
                            res["first_bad_expand"].append({"capacity": cap, "k": len(calls)})
                for _, rm, s, _, _ in calls:
                    seen[model.records(rm, s)] = True
                res["rm_forms"] |= {"every room" if c[1] is None else "room" for c in calls}
                res["sender_forms"] |= {"none" if c[2] is None else "slot" for c in calls}
                res["capacities"].append(cap)
                res["ks"].append(k)
                res["calls"] += 1
                res["items"] += len(calls) * cap
    res["records_seen"] = int(seen.sum())
    res["rm_forms"], res["sender_forms"] = sorted(res["rm_forms"]), sorted(res["sender_forms"])
    return res


def against_cpu(cpu: Cpu, r: device.Fanout, calls, model: Model) -> int:
    """Items of a Fanout of roster calls that differ from the restatement."""
    as_tables = [(t, None, int(rm is None), fl, com) for t, rm, s, fl, com in calls]
    return compare(r, expected(cpu, as_tables, [model.records(rm, s) for _, rm, s, _, _ in calls]), as_tables)[0]


def order_part(cpu: Cpu) -> dict:
    """plan_many, broadcast_many, an update of one slot, broadcast_many, plan_many on one roster; then two rosters
    used alternately."""
    cap = 300
    out = {"steps": [], "n_bad": 0}
    with device.Roster(cap) as roster:
        model = Model(cap)
        roster.update(range(cap), room=[j % 2 for j in range(cap)], colour=[j % 3 == 0 for j in range(cap)])
        model.update(range(cap), {"room": [j % 2 for j in range(cap)], "colour": [int(j % 3 == 0) for j in range(cap)]})
        calls = [(t, rm, 4, 0, device.COM_SHOUT) for t in devpath.line_texts("shout", 3) for rm in (0, None)]
        p1 = roster.plan_many(calls)
        saved = {f: np.copy(getattr(p1, f)) for f in PLAN_ARRAYS}
        out["steps"].append("plan_many")
        out["n_bad"] += len(plan_differences(cpu, p1, calls, model))
        f1 = roster.broadcast_many(calls)
        out["steps"].append("broadcast_many")
        out["n_bad"] += against_cpu(cpu, f1, calls, model) + (not same(p1.expand(), f1))
        roster.update([10], colour=1, ignshout=1, room=0)
        model.update([10], {"colour": 1, "ignshout": 1, "room": 0})
        out["steps"].append("update")
        f2 = roster.broadcast_many(calls)
        out["steps"].append("broadcast_many")
        out["n_bad"] += against_cpu(cpu, f2, calls, model)
        p2 = roster.plan_many(calls)
        out["steps"].append("plan_many")
        out["n_bad"] += len(plan_differences(cpu, p2, calls, model)) + (not same(p2.expand(), f2))
        out["update_changed_the_result"] = not same(f1, f2) and not np.array_equal(p1.admitted_bits, p2.admitted_bits)
        out["earlier_plan_unchanged"] = (all(np.array_equal(getattr(p1, f), v) for f, v in saved.items())
                                         and same(p1.expand(), f1))
    with device.Roster(300) as a, device.Roster(500) as b:
        ma, mb = Model(300), Model(500)
        a.update(range(300), room=[j % 3 for j in range(300)], colour=1)
        ma.update(range(300), {"room": [j % 3 for j in range(300)], "colour": 1})
        b.update(range(0, 500, 2), room=1, ignshout=1)
        mb.update(range(0, 500, 2), {"room": 1, "ignshout": 1})
        ca = [(t, 1, 4, 0, device.COM_SAY) for t in devpath.line_texts("say", 5)]
        cb = [(t, None, None, 1, device.COM_SHOUT) for t in devpath.line_texts("shout", 4)] + \
             [(b"~FRred\n", 1, None, 0, device.COM_SAY)]
        pa1 = a.plan_many(ca)
        pb1 = b.plan_many(cb)
        fa = a.broadcast_many(ca)
        pa2 = a.plan_many(ca)
        fb = b.broadcast_many(cb)
        pb2 = b.plan_many(cb)
        for p, m, calls in ((pa1, ma, ca), (pb1, mb, cb), (pa2, ma, ca), (pb2, mb, cb)):
            out["n_bad"] += len(plan_differences(cpu, p, calls, m))
        out["two_rosters_alternately_identical"] = (same(pa1.expand(), fa) and same(pa2.expand(), fa)
                                                    and same(pb1.expand(), fb) and same(pb2.expand(), fb))
        out["two_rosters_differ"] = pa1.expand().arena.tobytes() != pb1.expand().arena.tobytes()
    return out


def copies_part() -> dict:
    """h2d_bytes as device_roster_child.h2d_part reads them, through plan_many; d2h_bytes of the same texts to a
    roster that admits everyone and to one that admits nobody (every slot logging in)."""
    h2d = {"dirty": {}, "clean": {}, "after_update": {}, "clean_again": {}}
    calls = [(t, 0, 0, 0, device.COM_SAY) for t in devpath.line_texts("say", 10)]
    for cap in (256, 4096):
        with device.Roster(cap) as roster:
            roster.update(range(cap), room=0)
            h2d["dirty"][cap] = roster.plan_many(calls).timing["h2d_bytes"]
            h2d["clean"][cap] = roster.plan_many(calls).timing["h2d_bytes"]
            roster.update([5], colour=1)
            h2d["after_update"][cap] = roster.plan_many(calls).timing["h2d_bytes"]
            h2d["clean_again"][cap] = roster.plan_many(calls).timing["h2d_bytes"]
    cap = 1000
    calls = [(t, 0, None, 0, device.COM_SHOUT) for t in devpath.line_texts("shout", 20)]
    d2h = {"capacity": cap, "k": len(calls), "text_bytes": sum(len(c[0]) for c in calls)}
    for name, login in (("everyone", 0), ("nobody", 1)):
        with device.Roster(cap) as roster:
            roster.update(range(cap), room=0, login=login)
            p = roster.plan_many(calls)
            d2h[name] = p.timing["d2h_bytes"]
            d2h["admitted_" + name] = int(sum(p.admitted(k).sum() for k in range(len(calls))))
    return {"h2d": h2d, "d2h": d2h}


def bench_step(cpu: Cpu) -> dict:
    """The bench headline's step as a plan: 100 distinct .shout lines to 1000 slots in room 0, slot 0 the sender,
    colour on every other slot; and broadcast_many of the same call, for its d2h_bytes."""
    tab = devpath.listeners(1000, "half")
    with device.Roster(1000) as roster:
        roster.update(range(1000), room=0, colour=tab[:, device.LISTENER_FIELDS.index("colour")])
        calls = [(t, 0, 0, 0, device.COM_SHOUT) for t in devpath.line_texts("shout", 100)]
        p = roster.plan_many(calls)
        f = roster.broadcast_many(calls)
    as_tables = [(t, tab, 0, 0, device.COM_SHOUT) for t, _, _, _, _ in calls]
    rec = (tab.astype(np.int64) << np.arange(len(device.LISTENER_FIELDS))).sum(axis=1)
    bad, first = compare(p.expand(), expected(cpu, as_tables, [rec] * len(calls)), as_tables)
    bits = np.unpackbits(p.admitted_bits.view(np.uint8), bitorder="little")
    return {"broadcasts": len(calls), "deliveries": int(bits.sum()), "n_bad": bad + (not same(p.expand(), f)),
            "first_bad": first, "timing": p.timing, "fanout_d2h_bytes": f.timing["d2h_bytes"]}


def worst(cpu: Cpu) -> dict:
    """64 broadcasts of 1999 newlines to 64 slots with colour on, then a small call, then the large one again."""
    text = b"\n" * 1999
    with device.Roster(64) as roster:
        roster.update(range(64), room=0, colour=1)
        large = [(text, 0, None, 0, device.COM_SAY)] * 64
        a = roster.plan_many(large)
        roster.plan_many([(b"hi\n", 0, None, 0, device.COM_SAY)])
        b = roster.plan_many(large)
    rec = np.full(64, 2 | 4 | 64, dtype=np.int64)                        # has_room, same_room, colour
    as_tables = [(text, None, 0, 0, device.COM_SAY)] * 64
    bad, first = compare(a.expand(), expected(cpu, as_tables, [rec] * 64), as_tables)
    bad += sum(a.chunks(k, c) != cpu.chunks(text, c) for k in range(64) for c in (0, 1))
    pairs = sorted({tuple((int(a.variant_sizes[k, c]), int(a.write_counts[k, c])) for c in (0, 1)) for k in range(64)})
    ea, eb = a.expand(), b.expand()
    identical = same(ea, eb) and all(a.chunks(k, c) == b.chunks(k, c) for k in range(64) for c in (0, 1))
    return {"broadcasts": 64, "deliveries": int(ea.admitted.sum()), "variant_pairs": pairs,
            "cpu_pair": [(sum(map(len, cpu.chunks(text, c))), len(cpu.chunks(text, c))) for c in (0, 1)],
            "n_bad": int(bad), "first_bad": first, "reuse_identical": identical}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1401)
    ap.add_argument("--model-only", action="store_true", help="the random sequence's coverage, without a device")
    a = ap.parse_args()
    if a.model_only:
        # Roster.update and Model need no device; no call is made
        print("DEVICE_PLAN_MODEL " + json.dumps(random_part(Cpu(), a.seed, model_only=True)))
        return 0
    out = {"device_count": device.device_count()}
    if out["device_count"] < 1:
        print("device_plan_child: no GPU visible", file=sys.stderr)
        return 2
    cpu = Cpu()
    out["random"] = random_part(cpu, a.seed)
    out["order"] = order_part(cpu)
    out["copies"] = copies_part()
    out["bench_step"] = bench_step(cpu)
    out["worst"] = worst(cpu)
    print("DEVICE_PLAN " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
