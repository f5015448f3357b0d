"""The device work of tests/test_device_fanout.py, in a short-lived child process of its own.

A process that boots talkers never initialises HIP, so the test module starts this script once,
under ``timeout``, and asserts on the one JSON line it prints (``DEVICE_FANOUT {...}``).  Every check compares the
device's bytes AND write(2) chunk sizes with ``np_write_user_stream`` / ``np_fanout_admits`` of the CPU restatement,
called through its binding (nuts333_amd.nuts_path).

    python tests/device_fanout_child.py [--fuzz N]
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

from nuts333_amd import nuts_path  # noqa: E402

CODES = "RS OL UL LI RV FK FR FG FY FB FM FT FW BK BR BG BY BB BM BT BW".split()
WORDS = ["hello", "there", "nuts", "talker", "lines", "x", "yy", "zzz", "Scunthorpe", "42", "ok"]
TEXT_MAX = 1999


# ------------------------------------------------------------------ inputs
def markup_text(rng: random.Random) -> str:
    """Markup-dense text, after the generator of tests/test_differential_fuzz.py."""
    parts = []
    for _ in range(rng.randint(1, 12)):
        x = rng.random()
        if x < 0.20:
            parts.append("~" + rng.choice(CODES))
        elif x < 0.28:
            parts.append("/~" + rng.choice(["", "FR", "x", "/", "~"]))
        elif x < 0.36:
            parts.append(rng.choice(["~", "~~", "~F", "/", "//", "~zz", "\n", "~\n", "/\n"]))
        else:
            parts.append(rng.choice(WORDS))
    x = rng.random()
    if x < 0.05:
        parts.append("long" * rng.choice([50, 120, 230, 249]))
    return rng.choice([" ", "", "~"]).join(parts) + rng.choice(["", "", "\n", "?\n", "!"])


def boundary_text(rng: random.Random) -> str:
    """Long text that puts a newline / tilde / code / escape near the 994 and 1000 flush boundaries (and their
    second-buffer counterparts)."""
    head = "".join(rng.choice("ab ~/\n") if rng.random() < 0.05 else "a" for _ in range(rng.randint(960, 1010)))
    tail = "".join(rng.choice(["\n", "~", "~FR", "/~", "~RS", "b", "bb", "/~FR", "\n\n"]) for _ in range(rng.randint(1, 12)))
    rest = "".join(rng.choice(["c" * rng.randint(1, 400), "\n", "~OL", "/~", "~"]) for _ in range(rng.randint(0, 8)))
    return (head + tail + rest)[:TEXT_MAX]


def only_text(rng: random.Random) -> str:
    """Strings made only of '\\n', only of '~XX' (and stray '~'), or only of '/~'."""
    kind = rng.randrange(3)
    n = rng.choice([1, 2, 3, 100, 331, 332, 333, 498, 499, 500, 665, 666, 997, 999, TEXT_MAX])
    if kind == 0:
        s = "\n" * n
    elif kind == 1:
        s = "".join("~" + rng.choice(CODES) if rng.random() < 0.9 else "~" for _ in range(n))
    else:
        s = "/~" * n
    return s[:TEXT_MAX]


def random_bytes(rng: random.Random) -> bytes:
    alphabet = b"~/\n\r abRSOLFB" + bytes(range(1, 256))
    return bytes(rng.choice(alphabet) for _ in range(rng.randint(0, rng.choice([20, 200, TEXT_MAX]))))


def fuzz_items(seed: int, n: int):
    rng = random.Random(seed)
    items = []
    for _ in range(n):
        x = rng.random()
        if x < 0.80:
            t = markup_text(rng).encode()[:TEXT_MAX]
        elif x < 0.90:
            t = boundary_text(rng).encode()
        elif x < 0.95:
            t = only_text(rng).encode()
        else:
            t = random_bytes(rng)
        items.append((t, rng.randrange(2)))
    return items


# ------------------------------------------------------------------ checks
def compare_batch(dev, items, batch: int = 50_000) -> dict:
    from nuts333_amd import device
    bad, n_bad, total_bytes, total_writes, worst_bytes, worst_writes = [], 0, 0, 0, 0, 0
    for lo in range(0, len(items), batch):
        part = items[lo:lo + batch]
        r = dev.transduce_batch([t for t, _ in part], [c for _, c in part])
        for j, (t, c) in enumerate(part):
            got = device.chunks(r, j)
            want = nuts_path.chunks(t, c)
            nb = sum(map(len, got))
            total_bytes += nb
            total_writes += len(got)
            worst_bytes = max(worst_bytes, nb - device.max_bytes(len(t)))
            worst_writes = max(worst_writes, len(got))
            if got != want or not r.admitted[j]:
                n_bad += 1
                if len(bad) < 5:
                    bad.append({"text": t[:200].decode("latin-1"), "len": len(t), "colour": c,
                                "device_sizes": [len(x) for x in got], "cpu_sizes": [len(x) for x in want]})
    return {"items": len(items), "n_bad": n_bad, "first_bad": bad, "bytes": total_bytes, "writes": total_writes,
            "max_bytes_minus_bound": worst_bytes, "max_writes": worst_writes}


def vectors(dev) -> dict:
    from nuts333_amd import device
    doc = json.loads((REPO / "tests" / "golden" / "vectors" / "transducer.json").read_text())
    texts, colours, expect = [], [], []
    for v in doc["vectors"]:
        text = ("Bobby says: " + v["line"] + "\n").encode("latin-1")
        for colour, key in ((1, "colour_on"), (0, "colour_off")):
            texts.append(text)
            colours.append(colour)
            expect.append(v[key].encode("latin-1"))
    r = dev.transduce_batch(texts, colours)
    concat_bad = [i for i in range(len(texts)) if r.output(i) != expect[i]]
    chunk_bad = [i for i in range(len(texts)) if device.chunks(r, i) != nuts_path.chunks(texts[i], colours[i])]
    return {"vectors": len(doc["vectors"]), "items": len(texts), "concat_bad": concat_bad[:10],
            "n_concat_bad": len(concat_bad), "n_chunk_bad": len(chunk_bad)}


def predicate(dev) -> dict:
    """All 2^6 listener states x rm_is_null x force_listen x {SAY, SHOUT, SEMOTE}: one 64-listener broadcast each."""
    from nuts333_amd import device
    text = b"~OLUaaa shouts:~RS hello /~ there\n"
    states = [[(s >> k) & 1 for k in range(6)] for s in range(64)]
    cases = bad = 0
    first = []
    for rm_is_null in (0, 1):
        for force_listen in (0, 1):
            for com in (device.COM_SAY, device.COM_SHOUT, device.COM_SEMOTE):
                table = [st + [st[0] ^ st[3]] for st in states]          # colour varied too
                r = dev.broadcast(text, table, rm_is_null, force_listen, com)
                for i, st in enumerate(states):
                    cases += 1
                    want = nuts_path.admits(st, rm_is_null, force_listen, com)
                    out = device.chunks(r, i)
                    ok = bool(r.admitted[i]) == want and out == (nuts_path.chunks(text, table[i][6]) if want else [])
                    if not ok:
                        bad += 1
                        if len(first) < 5:
                            first.append({"state": st, "rm_is_null": rm_is_null, "force_listen": force_listen,
                                          "com": com, "device": bool(r.admitted[i]), "cpu": want})
    return {"cases": cases, "n_bad": bad, "first_bad": first}


def broadcast_1000(dev) -> dict:
    """1000 listeners, mixed colour and ignshout, the sender among them, a few logging in / elsewhere: a .shout."""
    from nuts333_amd import device
    rng = random.Random(1410)
    text = b"~OLUaaa shouts:~RS synthetic /~ broadcast ~FRline~RS 000123\n"
    table = []
    for i in range(1000):
        table.append([int(rng.random() < 0.02), int(rng.random() < 0.98), int(rng.random() < 0.5), int(rng.random() < 0.05),
                      int(rng.random() < 0.25), int(i == 417), rng.randrange(2)])
    r = dev.broadcast(text, table, 1, 0, device.COM_SHOUT)
    want_admit, bad = [], 0
    for i, row in enumerate(table):
        a = nuts_path.admits(row[:6], 1, 0, device.COM_SHOUT)
        want_admit.append(a)
        if bool(r.admitted[i]) != a or device.chunks(r, i) != (nuts_path.chunks(text, row[6]) if a else []):
            bad += 1
    return {"listeners": 1000, "admitted": int(r.admitted.sum()), "cpu_admitted": sum(want_admit),
            "sender_admitted": bool(r.admitted[417]), "n_bad": bad, "bytes": int(r.out_offsets[-1]),
            "timing": r.timing}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--fuzz", type=int, default=200_000)
    ap.add_argument("--seed", type=int, default=333)
    a = ap.parse_args()
    from nuts333_amd import device
    out = {"device_count": device.device_count()}
    if out["device_count"] < 1:
        print("device_fanout_child: no GPU visible", file=sys.stderr)
        return 2
    out["vectors"] = vectors(device)
    worst = [("\n" * TEXT_MAX).encode(), ("~RS" * 666).encode()]
    out["worst"] = compare_batch(device, [(worst[0], 1), (worst[0], 0), (worst[1], 0), (worst[1], 1)])
    r = device.transduce_batch([worst[0], worst[1]], [1, 0])
    out["worst"]["newlines_colour_on"] = [int(r.out_offsets[1]), int(r.write_offsets[1])]
    out["worst"]["codes_colour_off"] = [int(r.out_offsets[2] - r.out_offsets[1]), int(r.write_offsets[2] - r.write_offsets[1])]
    out["fuzz"] = compare_batch(device, fuzz_items(a.seed, a.fuzz))
    out["predicate"] = predicate(device)
    out["broadcast"] = broadcast_1000(device)
    print("DEVICE_FANOUT " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
