"""The device work of tests/test_device_broadcast_many.py, in a short-lived child process of its own.

As tests/device_fanout_child.py: the test module starts this script once, under ``timeout``, and asserts on the one
JSON line it prints (``DEVICE_MANY {...}``).  Every check compares ``device.broadcast_many`` with the CPU restatement
through its binding (``nuts_path.admits`` / ``nuts_path.chunks``): admit flags, bytes and write(2) chunk sizes.  The CPU
chunks are computed once per (text, colour) and the predicate once per (record, rm_is_null, force_listen, command),
since items share them.

    python tests/device_many_child.py [--seed S]
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
from nuts333_amd import devpath, device, nuts_path  # noqa: E402

KS = (1, 2, 7, 64, 300, 1000)
COMS = (device.COM_SAY, device.COM_SHOUT, device.COM_SEMOTE)
BITS = np.arange(len(device.LISTENER_FIELDS))


class Cpu:
    """What the restatement says, memoised."""

    def __init__(self):
        self._chunks, self._admit = {}, {}

    def chunks(self, text: bytes, colour: int) -> list[bytes]:
        if (text, colour) not in self._chunks:
            self._chunks[text, colour] = nuts_path.chunks(text, colour)
        return self._chunks[text, colour]

    def admit(self, rm_is_null: int, force_listen: int, com: int) -> np.ndarray:
        """bool[128]: np_fanout_admits for every listener record (its low six bits are struct np_listener)."""
        key = (rm_is_null, force_listen, com)
        if key not in self._admit:
            states = [nuts_path.admits([(r >> b) & 1 for b in range(6)], rm_is_null, force_listen, com)
                      for r in range(64)]
            self._admit[key] = np.array(states * 2, dtype=bool)
        return self._admit[key]


def table(records: np.ndarray) -> np.ndarray:
    """Listener records (bit k = LISTENER_FIELDS[k]) -> the (N, 7) table broadcast() takes."""
    return ((records[:, None] >> BITS) & 1).astype(np.uint8)


def expected(cpu: Cpu, calls, records) -> dict:
    """Admit flags, bytes, item sizes, chunk sizes and chunk counts of a broadcast_many call, from the restatement."""
    admit, parts, sizes, wsz, nw = [], [], [], [], []
    for (text, _, rm_is_null, force_listen, com), rec in zip(calls, records):
        a = cpu.admit(rm_is_null, force_listen, com)[rec]
        var = [cpu.chunks(text, 0), cpu.chunks(text, 1), []]
        joined = [b"".join(v) for v in var]
        lens = [[len(c) for c in v] for v in var]
        sel = np.where(a, (rec >> 6) & 1, 2).tolist()
        admit.append(a)
        parts.extend(joined[s] for s in sel)
        sizes.extend(len(joined[s]) for s in sel)
        for s in sel:
            wsz.extend(lens[s])
            nw.append(len(lens[s]))
    return {"admitted": np.concatenate(admit), "arena": b"".join(parts), "sizes": np.array(sizes, dtype=np.int64),
            "write_sizes": np.array(wsz, dtype=np.int32), "writes": np.array(nw, dtype=np.int64)}


def compare(r: device.Fanout, want: dict, calls) -> tuple[int, list]:
    """Items that differ in admit flag, bytes or chunk sizes (whole-array checks first; per item only on a difference)."""
    m = len(want["admitted"])
    out_off = np.concatenate([[0], np.cumsum(want["sizes"])])
    w_off = np.concatenate([[0], np.cumsum(want["writes"])])
    if (len(r.admitted) == m and np.array_equal(r.admitted, want["admitted"]) and np.array_equal(r.out_offsets, out_off)
            and np.array_equal(r.write_offsets, w_off) and r.arena.tobytes() == want["arena"]
            and np.array_equal(r.write_sizes, want["write_sizes"])):
        return 0, []
    bad, first = 0, []
    owner = np.repeat(np.arange(len(calls)), np.diff(r.broadcast_offsets))
    for i in range(min(m, len(r.admitted))):
        want_bytes = want["arena"][out_off[i]:out_off[i + 1]]
        want_sizes = want["write_sizes"][w_off[i]:w_off[i + 1]].tolist()
        got_sizes = r.write_sizes[r.write_offsets[i]:r.write_offsets[i + 1]].tolist()
        if bool(r.admitted[i]) != bool(want["admitted"][i]) or r.output(i) != want_bytes or got_sizes != want_sizes:
            bad += 1
            if len(first) < 5:
                k = int(owner[i])
                first.append({"item": i, "broadcast": k, "text": calls[k][0][:120].decode("latin-1"),
                              "len": len(calls[k][0]), "device_admitted": bool(r.admitted[i]),
                              "cpu_admitted": bool(want["admitted"][i]), "device_sizes": got_sizes,
                              "cpu_sizes": want_sizes})
    return max(bad, abs(m - len(r.admitted))), first


def random_calls(rng: random.Random, nrng: np.random.Generator, texts, k: int):
    """k broadcasts: N in [1, 1500], every listener record 0..127 at random, random flags and command; the call is
    kept under MANY_ARENA_CAP by trimming its largest tables."""
    calls, records = [], []
    for _ in range(k):
        text = next(texts)
        rec = nrng.integers(0, 128, size=rng.randint(1, 1500))
        records.append(rec)
        calls.append([text, None, rng.randrange(2), rng.randrange(2), rng.choice(COMS)])
    while sum(len(r) * device.max_bytes(len(c[0])) for c, r in zip(calls, records)) > device.MANY_ARENA_CAP:
        j = max(range(k), key=lambda i: len(records[i]) * len(calls[i][0]))
        records[j] = records[j][:max(1, len(records[j]) // 2)]
    for c, r in zip(calls, records):
        c[1] = table(r)
    return [tuple(c) for c in calls], records


def random_part(cpu: Cpu, seed: int) -> tuple[dict, dict]:
    """Two rounds over KS; the first round's broadcasts also go through K single broadcast() calls."""
    rng, nrng = random.Random(seed), np.random.default_rng(seed)
    pool = [t for t, _ in fuzz_items(seed, 2 * sum(KS))]
    texts = iter(pool)
    res = {"ks": [], "broadcasts": 0, "items": 0, "n_bad": 0, "first_bad": [], "records_seen": 0,
           "long_texts": sum(len(t) >= 994 for t in pool)}
    singles = {"broadcasts": 0, "items": 0, "n_bad": 0, "first_bad": []}
    seen = np.zeros(128, dtype=bool)
    for rnd in range(2):
        for k in KS:
            calls, records = random_calls(rng, nrng, texts, k)
            r = device.broadcast_many(calls)
            bad, first = compare(r, expected(cpu, calls, records), calls)
            res["ks"].append(k)
            res["broadcasts"] += k
            res["items"] += len(r.admitted)
            res["n_bad"] += bad
            res["first_bad"] += first[:5 - len(res["first_bad"])]
            for rec in records:
                seen[rec] = True
            if rnd == 0:
                single_vs_many(r, calls, singles)
    res["records_seen"] = int(seen.sum())
    return res, singles


def single_vs_many(r: device.Fanout, calls, out: dict) -> None:
    """Broadcast k of the many-call result, slice by slice, against one broadcast() of the same arguments."""
    bo = r.broadcast_offsets
    for k, call in enumerate(calls):
        s = device.broadcast(*call)
        lo, hi = int(bo[k]), int(bo[k + 1])
        o0, w0 = int(r.out_offsets[lo]), int(r.write_offsets[lo])
        same = (np.array_equal(r.admitted[lo:hi], s.admitted)
                and np.array_equal(r.out_offsets[lo:hi + 1] - o0, s.out_offsets)
                and np.array_equal(r.write_offsets[lo:hi + 1] - w0, s.write_offsets)
                and np.array_equal(r.arena[o0:int(r.out_offsets[hi])], s.arena)
                and np.array_equal(r.write_sizes[w0:int(r.write_offsets[hi])], s.write_sizes))
        out["broadcasts"] += 1
        out["items"] += hi - lo
        if not same:
            out["n_bad"] += 1
            if len(out["first_bad"]) < 5:
                out["first_bad"].append({"broadcast": k, "listeners": hi - lo, "text": call[0][:120].decode("latin-1")})


def bench_step(cpu: Cpu) -> dict:
    """The bench headline's step: 100 distinct .shout lines to 1000 listeners, colour on every other one."""
    tab = devpath.listeners(1000, "half")
    calls = [(t, tab, 0, 0, device.COM_SHOUT) for t in devpath.line_texts("shout", 100)]
    rec = (tab.astype(np.int64) << BITS).sum(axis=1)
    r = device.broadcast_many(calls)
    bad, first = compare(r, expected(cpu, calls, [rec] * len(calls)), calls)
    return {"broadcasts": len(calls), "deliveries": int(r.admitted.sum()), "bytes": int(r.out_offsets[-1]),
            "n_bad": bad, "first_bad": first, "timing": r.timing}


def worst(cpu: Cpu) -> dict:
    """64 broadcasts of 1999 newlines, colour on (the largest output per item), then a small call, then the large one
    again: the device buffers are reused and must give the same result."""
    text = b"\n" * 1999
    rec = np.full(64, 2 | 4 | 64, dtype=np.int64)                        # has_room, same_room, colour
    large = [(text, table(rec), 0, 0, device.COM_SAY)] * 64
    a = device.broadcast_many(large)
    bad, first = compare(a, expected(cpu, large, [rec] * 64), large)
    device.broadcast_many([(b"hi\n", table(rec[:3]), 0, 0, device.COM_SAY)])
    b = device.broadcast_many(large)
    same = all(np.array_equal(getattr(a, f), getattr(b, f))
               for f in ("admitted", "out_offsets", "arena", "write_offsets", "write_sizes", "broadcast_offsets"))
    return {"items": len(a.admitted), "per_item": sorted({(int(x), int(y)) for x, y in
                                                           zip(np.diff(a.out_offsets), np.diff(a.write_offsets))}),
            "n_bad": bad, "first_bad": first, "reuse_identical": same}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1321)
    a = ap.parse_args()
    out = {"device_count": device.device_count()}
    if out["device_count"] < 1:
        print("device_many_child: no GPU visible", file=sys.stderr)
        return 2
    cpu = Cpu()
    out["random"], out["singles"] = random_part(cpu, a.seed)
    out["bench_step"] = bench_step(cpu)
    out["worst"] = worst(cpu)
    print("DEVICE_MANY " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
