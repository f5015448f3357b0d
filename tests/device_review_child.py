"""The device work of tests/test_device_review.py, in a short-lived child process of its own, and the CPU models the
host tier of that module shares with it.

As tests/device_plan_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_REVIEW {...}``).  ``Rings`` is the CPU model of a roster's review rings: ``np_record`` of the
restatement per recorded broadcast, and ``nuts_path.chunks`` per stored line for a review.  Every ``review_many`` of the
random histories is compared with it in full: every line, both variants, every chunk size.  ``local_rule`` is a numpy
model of the rule nuts_roster_review applies to a line whose output stays at or below 994 bytes.

    python tests/device_review_child.py [--seed S]
"""
from __future__ import annotations

import argparse
import ctypes
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

LINES, SLOT = device.REVIEW_LINES, device.REVIEW_LEN + 2
RESET = b"\x1b[0m"
#: a line's output up to here cannot flush in mid-line (the flush test is pos > NP_OUT_BUFF - 6)
WAVE_LIMIT = 1000 - 6
COLCOM = ("RS", "OL", "UL", "LI", "RV", "FK", "FR", "FG", "FY", "FB", "FM", "FT", "FW", "BK", "BR", "BG", "BY", "BB",
          "BM", "BT", "BW")
COLARG = ("0", "1", "4", "5", "7", "30", "31", "32", "33", "34", "35", "36", "37", "40", "41", "42", "43", "44", "45",
          "46", "47")


# ------------------------------------------------------------------ the CPU model of the rings
class Rings:
    """``rooms`` review rings as the talker keeps them: np_record to store, clear_revbuff to clear, .review to read."""

    def __init__(self, rooms: int):
        self.ring = [ctypes.create_string_buffer(LINES * SLOT) for _ in range(rooms)]
        self.revline = [ctypes.c_int(0) for _ in range(rooms)]

    def record(self, rm: int, text: bytes) -> None:
        nuts_path.lib().np_record(self.ring[rm], LINES, ctypes.byref(self.revline[rm]), text)

    def clear(self, rm: int) -> None:
        for i in range(LINES):
            self.ring[rm][i * SLOT] = b"\0"
        self.revline[rm].value = 0

    def lines(self, rm: int) -> list[bytes]:
        """The non-empty lines from the cursor onwards: what .review passes to write_user, one call each."""
        raw, rev = self.ring[rm].raw, self.revline[rm].value
        slots = [raw[s * SLOT:(s + 1) * SLOT].split(b"\0", 1)[0] for s in ((rev + i) % LINES for i in range(LINES))]
        return [line for line in slots if line]

    def chunks(self, rm: int, colour: int) -> list[bytes]:
        return [c for line in self.lines(rm) for c in nuts_path.chunks(line, colour)]


def sequential_expected(lines, cache: dict) -> int:
    """How many (line, variant) pairs have an output past WAVE_LIMIT, the reset apart: those the kernel hands to its
    sequential transducer."""
    n = 0
    for line in lines:
        if line not in cache:
            cache[line] = sum(len(nuts_path.transduce(line, c)) - 4 * c > WAVE_LIMIT for c in (0, 1))
        n += cache[line]
    return n


# ------------------------------------------------------------------ the local rule, in numpy
def local_rule(lines, colour: int):
    """The rule of nuts_roster_review's wave path over a batch of lines (each at most 201 bytes, no NUL): a byte's output
    from the bytes i-3 .. i+2 alone.  Returns the outputs without the trailing reset, concatenated, and their sizes."""
    n, width = len(lines), max(1, max((len(x) for x in lines), default=0))
    s = np.zeros((n, width + 5), dtype=np.uint8)              # three bytes of 0 before the line, two after it
    for r, x in enumerate(lines):
        s[r, 3:3 + len(x)] = np.frombuffer(x, dtype=np.uint8)
    at = lambda d: s[:, 3 + d:3 + d + width]                  # the byte d places after byte i
    pairs = np.array([ord(a) << 8 | ord(b) for a, b in COLCOM], dtype=np.int64)
    which = lambda d: np.where((at(d) == ord("~")) & (at(d - 1) != ord("/")),
                               at(d + 1).astype(np.int64) << 8 | at(d + 2), -1)
    command = lambda d: (which(d)[..., None] == pairs).any(axis=-1)     # a command tilde d places after byte i
    ch = at(0)
    consumed = command(-1) | command(-2)
    own = (which(0)[..., None] == pairs)
    is_cmd, index = own.any(axis=-1), own.argmax(axis=-1)
    out = np.zeros((n, width, 6), dtype=np.uint8)
    size = np.ones((n, width), dtype=np.int64)
    out[..., 0] = ch
    newline = ch == ord("\n")
    if colour:
        out[newline, :] = np.frombuffer(RESET + b"\n\r", dtype=np.uint8)
        size[newline] = 6
        codes = np.zeros((len(COLARG), 6), dtype=np.uint8)
        for i, arg in enumerate(COLARG):
            code = f"\x1b[{arg}m".encode()
            codes[i, :len(code)] = np.frombuffer(code, dtype=np.uint8)
        out[is_cmd, :] = codes[index[is_cmd]]
        size[is_cmd] = np.array([3 + len(a) for a in COLARG])[index[is_cmd]]
    else:
        out[newline, :2] = np.frombuffer(b"\n\r", dtype=np.uint8)
        size[newline] = 2
        size[is_cmd] = 0
    size[(ch == ord("/")) & (at(1) == ord("~"))] = 0
    size[consumed | (ch == 0)] = 0
    keep = np.arange(6) < size[..., None]
    return out[keep].tobytes(), size.sum(axis=1)


# ------------------------------------------------------------------ texts
def special_texts() -> list[bytes]:
    doc = json.loads((REPO / "tests" / "golden" / "vectors" / "transducer.json").read_text())
    vectors = [("Bobby says: " + v["line"] + "\n").encode("latin-1") for v in doc["vectors"]]
    return [b"", b"x" * 199, b"y" * 200, b"z" * 201, b"\n" * 1999, b"\n" * 200, b"\n" * 199, b"\n" * 166 + b"tail",
            b"\n" * 165 + b"abcd", b"\n" * 165 + b"abcde", b"a" * 30 + b"\n" * 170, b"~FR\n" * 50,
            b"x" * 198 + b"~FRstraddles byte 200\n", b"x" * 199 + b"~FRtilde at 199\n", b"x" * 197 + b"~FRfits\n",
            b"x" * 199 + b"/~FRslash at the cut\n", b"x" * 198 + b"/~FRslash before the cut\n",
            b"~OLUaaa shouts:~RS hello /~FR there\n", b"Uaaa says: hi\n", b"~", b"~F", b"/", b"\n"] + vectors


def same_review(a: device.Review, qa: int, b: device.Review, qb: int) -> bool:
    return (a.lines(qa) == b.lines(qb) and a.line_counts[qa] == b.line_counts[qb]
            and all(a.chunks(qa, c) == b.chunks(qb, c) and a.variant(qa, c) == b.variant(qb, c) for c in (0, 1)))


def review_differences(rv: device.Review, rooms, model: Rings, counts: dict, cache: dict) -> list:
    """What of a Review differs from the model: every room, every line, both variants, every chunk size."""
    bad = []
    if rv.rooms.tolist() != list(rooms):
        bad.append({"what": "rooms"})
    for q, rm in enumerate(rooms):
        want = model.lines(rm)
        counts["rooms_reviewed"] += 1
        counts["lines_compared"] += len(want)
        seq = sequential_expected(want, cache)
        counts["sequential_lines"] += seq
        counts["wave_lines"] += 2 * len(want) - seq
        if rv.lines(q) != want or int(rv.line_counts[q]) != len(want):
            bad.append({"what": "lines", "room": rm, "device": len(rv.lines(q)), "cpu": len(want)})
        if int(rv.sequential[q]) != seq:
            bad.append({"what": "sequential path count", "room": rm, "device": int(rv.sequential[q]), "cpu": seq})
        for c in (0, 1):
            ch = model.chunks(rm, c)
            n = int(rv.write_counts[q, c])
            if (rv.variant(q, c) != b"".join(ch) or n != len(ch)
                    or rv.write_sizes[q, c, :n].tolist() != [len(x) for x in ch] or rv.chunks(q, c) != ch):
                bad.append({"what": "variant", "room": rm, "colour": c, "device_bytes": int(rv.variant_sizes[q, c]),
                            "cpu_bytes": sum(map(len, ch)), "device_writes": n, "cpu_writes": len(ch)})
    return bad


def plan_differences(p: device.Plan, t: device.Plan) -> int:
    """Fields of a plan made with ``record`` that differ from its twin's, made without."""
    bad = sum(not np.array_equal(getattr(p, f), getattr(t, f))
              for f in ("admitted_bits", "colour_bits", "variant_starts", "variant_sizes", "write_counts"))
    for k in range(len(p.admitted_bits)):
        for c in (0, 1):
            n = int(p.write_counts[k, c])
            bad += p.variant(k, c) != t.variant(k, c) or p.write_sizes[k, c, :n].tolist() != t.write_sizes[k, c, :n].tolist()
    return int(bad) + (p.capacity != t.capacity)


# ------------------------------------------------------------------ the parts
ROSTERS = ((1, 1), (2, 7), (15, 100), (16, 1000), (device.MAX_REVIEW_ROOMS, 64))   # (review_rooms, capacity)
KS = (1, 7, 100, 1000)


def random_part(seed: int) -> dict:
    rng = random.Random(seed)
    pool = special_texts() + [t for t, _ in fuzz_items(seed, 600)]
    counts = {"calls": 0, "record_modes": set(), "ks": set(), "rooms_reviewed": 0, "lines_compared": 0,
              "sequential_lines": 0, "wave_lines": 0, "updates": 0, "clears": 0, "fanouts": 0, "reviews": 0,
              "most_records_into_one_room_in_one_call": 0, "duplicate_rooms_reviewed": 0, "texts_recorded": set()}
    res = {"rosters": [], "n_bad": 0, "first_bad": [], "n_bad_plan": 0}
    cache: dict = {}

    def check(rv, rooms, model):
        bad = review_differences(rv, rooms, model, counts, cache)
        res["n_bad"] += len(bad)
        res["first_bad"] += bad[:5 - len(res["first_bad"])]
        counts["reviews"] += 1

    for rr, cap in ROSTERS:
        res["rosters"].append([rr, cap])
        hot = sorted({0, rr // 2, rr - 1})                       # most records go to a few rooms, so that rings wrap
        with device.Roster(cap, review_rooms=rr) as roster, device.Roster(cap) as twin:
            model = Rings(rr)
            ops = ["plan"] * 5 + ["review"] * 3 + ["update", "clear", "fanout"]
            steps = [("plan", k) for k in KS] + [(rng.choice(ops), rng.choice(KS)) for _ in range(14)]
            rng.shuffle(steps)
            for op, k in steps:
                if op == "update":
                    slots = [rng.randrange(cap) for _ in range(rng.randint(1, 5))]
                    fields = {"room": [rng.choice((0, 1, None)) for _ in slots], "colour": rng.randrange(2)}
                    roster.update(slots, **fields)
                    twin.update(slots, **fields)
                    counts["updates"] += 1
                elif op == "clear":
                    rooms = [rng.choice(hot + [rng.randrange(rr)]) for _ in range(rng.randint(1, 3))]
                    roster.clear_review(rooms)
                    for rm in rooms:
                        model.clear(rm)
                    counts["clears"] += 1
                elif op == "fanout":
                    roster.broadcast_many([(rng.choice(pool)[:300], rng.choice((0, None)), None, 0, device.COM_SAY)
                                           for _ in range(3)])
                    counts["fanouts"] += 1
                elif op == "review":
                    rooms = [rng.choice(hot + [rng.randrange(rr)]) for _ in range(rng.randint(1, 6))]
                    counts["duplicate_rooms_reviewed"] += len(rooms) - len(set(rooms))
                    check(roster.review_many(rooms), rooms, model)
                else:
                    mode = rng.choice(("none", "all", "mix"))
                    calls, record = [], []
                    for _ in range(k):
                        on = mode == "all" or (mode == "mix" and rng.random() < 0.5)
                        rm = rng.choice(hot + [rng.randrange(rr)]) if on else rng.choice((None, 0, rr + 5))
                        calls.append((rng.choice(pool), rm, rng.choice((None, rng.randrange(cap))), rng.randrange(2),
                                      device.COM_SAY))
                        record.append(on)
                    arg = {"none": None, "all": True, "mix": record}[mode]
                    p = roster.plan_many(calls, record=arg)
                    res["n_bad_plan"] += plan_differences(p, twin.plan_many(calls))
                    per_room: dict = {}
                    for (text, rm, *_), on in zip(calls, record):
                        if on:
                            model.record(rm, text)
                            per_room[rm] = per_room.get(rm, 0) + 1
                            counts["texts_recorded"].add(text)
                    counts["most_records_into_one_room_in_one_call"] = max(
                        [counts["most_records_into_one_room_in_one_call"], *per_room.values()])
                    counts["calls"] += 1
                    counts["record_modes"].add(mode)
                    counts["ks"].add(k)
            everything = list(range(rr))
            check(roster.review_many(everything), everything, model)
    specials = special_texts()
    counts["special_texts_recorded"] = sum(t in counts["texts_recorded"] for t in specials)
    counts["special_texts"] = len(specials)
    del counts["texts_recorded"]
    counts["record_modes"], counts["ks"] = sorted(counts["record_modes"]), sorted(counts["ks"])
    return {**res, **counts}


def specials_part() -> dict:
    """Every special text recorded once, in a room of its own turn, 15 to a ring, and reviewed at once; then all of them
    into one room in one call, so that only the last 15 survive."""
    texts = special_texts()
    rr = (len(texts) + LINES - 1) // LINES
    counts = {"rooms_reviewed": 0, "lines_compared": 0, "sequential_lines": 0, "wave_lines": 0}
    with device.Roster(8, review_rooms=rr + 1) as roster:
        model = Rings(rr + 1)
        calls = [(t, i // LINES, None, 0, device.COM_SAY) for i, t in enumerate(texts)]
        roster.plan_many(calls, record=True)
        for t, rm, *_ in calls:
            model.record(rm, t)
        bad = review_differences(roster.review_many(range(rr)), list(range(rr)), model, counts, {})
        roster.plan_many([(t, rr, None, 0, device.COM_SAY) for t in texts], record=True)
        for t in texts:
            model.record(rr, t)
        bad += review_differences(roster.review_many([rr]), [rr], model, counts, {})
    return {"texts": len(texts), "n_bad": len(bad), "first_bad": bad[:5], **counts}


def order_part() -> dict:
    texts = devpath.line_texts("say", 40) + [b"", b"q" * 250]
    calls = [(t, i % 3, None, 0, device.COM_SAY) for i, t in enumerate(texts)]
    out = {}
    with device.Roster(10, review_rooms=4) as a, device.Roster(10, review_rooms=4) as b:
        a.plan_many(calls, record=True)
        for c in calls:
            b.plan_many([c], record=True)
        ra, rb = a.review_many(range(4)), b.review_many(range(4))
        out["one_call_equals_k_calls"] = all(same_review(ra, q, rb, q) for q in range(4))
        out["line_counts"] = ra.line_counts.tolist()
        saved = {f: np.copy(getattr(ra, f)) for f in ("rooms", "line_counts", "stored", "variants", "variant_starts",
                                                      "variant_sizes", "write_counts", "write_sizes")}
        # a clear between two calls empties exactly those rooms
        a.clear_review([1])
        rc = a.review_many(range(4))
        out["cleared_room_is_empty"] = int(rc.line_counts[1]) == 0 and rc.variant(1, 0) == b"" and rc.chunks(1, 1) == []
        out["other_rooms_kept"] = all(same_review(rc, q, ra, q) for q in (0, 2, 3))
        # a pending clear takes effect before the records of the next recording call, and survives a plain call
        a.clear_review(0)
        a.plan_many(calls[:5])
        a.plan_many([(b"after the clear\n", 0, None, 0, device.COM_SAY)], record=[True])
        rd = a.review_many([0, 2, 0])
        out["clear_then_record"] = rd.lines(0) == [b"after the clear\n"] and same_review(rd, 0, rd, 2)
        out["room_2_still_kept"] = same_review(rd, 1, ra, 2)
        # the review taken first is what it was: its arrays are its own
        out["earlier_review_unchanged"] = all(np.array_equal(getattr(ra, f), v) for f, v in saved.items())
        out["later_review_differs"] = not same_review(rd, 0, ra, 0)
    return out


def copies_part() -> dict:
    """Copy volume of review_many by Q, over full and over empty rings; of plan_many with and without rings."""
    out = {"review": {}, "plan": {}}
    full = [(b"\n" * 200, rm, None, 0, device.COM_SAY) for rm in range(64) for _ in range(LINES)]
    for q in (1, 5, 64):
        with device.Roster(100, review_rooms=64) as empty, device.Roster(100, review_rooms=64) as filled:
            filled.plan_many(full, record=True)
            e, f = empty.review_many(range(q)), filled.review_many(range(q))
            out["review"][q] = {"empty": [e.timing["h2d_bytes"], e.timing["d2h_bytes"]],
                                "full": [f.timing["h2d_bytes"], f.timing["d2h_bytes"]],
                                "full_bytes": int(f.variant_sizes.sum()), "empty_bytes": int(e.variant_sizes.sum())}
    calls = [(t, 0, 0, 0, device.COM_SAY) for t in devpath.line_texts("say", 10)]
    for name, rr in (("without_rings", 0), ("with_rings", 16)):
        with device.Roster(256, review_rooms=rr) as roster:
            roster.update(range(256), room=0)
            dirty, clean = roster.plan_many(calls).timing, roster.plan_many(calls).timing
            t = {"dirty": [dirty["h2d_bytes"], dirty["d2h_bytes"]], "clean": [clean["h2d_bytes"], clean["d2h_bytes"]]}
            if rr:
                rec = roster.plan_many(calls, record=True).timing
                t["recording"] = [rec["h2d_bytes"], rec["d2h_bytes"]]
                after = roster.plan_many(calls).timing
                t["clean_after_recording"] = [after["h2d_bytes"], after["d2h_bytes"]]
            out["plan"][name] = t
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1501)
    a = ap.parse_args()
    out = {"device_count": device.device_count()}
    if out["device_count"] < 1:
        print("device_review_child: no GPU visible", file=sys.stderr)
        return 2
    out["specials"] = specials_part()
    out["random"] = random_part(a.seed)
    out["order"] = order_part()
    out["copies"] = copies_part()
    print("DEVICE_REVIEW " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
