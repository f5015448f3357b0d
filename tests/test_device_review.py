"""Review rings of a resident roster: ``Roster(capacity, review_rooms)``, ``plan_many(record=)``, ``clear_review``,
``review_many``, ``device.Review`` and nuts_roster_record / nuts_roster_review of fanout.hip.

Host tier (unmarked): everything malformed is rejected before the device library loads; the CPU model of the rings
(``Rings`` of tests/device_review_child.py: ``np_record`` + ``nuts_path.chunks`` per line) reproduces the session the
reference recorded in tests/golden/review.json; the per-line bounds the buffers are sized by hold on the restatement at
their worst cases; a ``Review`` built by hand obeys its contract; the local rule of the review kernel's wave path
(``local_rule``, numpy) equals ``nuts_path.transduce`` on 120,000 seeded lines wherever the output stays at or below 994
bytes.  The kernels' scratch-free compile is tests/test_device_fanout.py's, over every name in ``device.KERNELS``.

The corner cases of record()'s strncpy (nuts333.c:2066-2069), by name: a text of 200 bytes or more is cut to 200 and
gets a forced newline (a 201-byte line); a shorter text is stored as it is; an empty text stores an empty line, which
.review skips, yet it advances the cursor and overwrites the oldest line.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_review_child.py, under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import json
import random
from pathlib import Path

import numpy as np
import pytest

import child_run
from device_review_child import RESET, WAVE_LIMIT, Rings, local_rule, special_texts
from nuts333_amd import device, nuts_path

REPO = Path(__file__).resolve().parent.parent
SAY = device.COM_SAY
GOOD = (b"hello\n", 0, None, 0, SAY)


# ------------------------------------------------------------------ host tier
@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


def test_the_new_kernels_are_listed():
    assert {"nuts_roster_record", "nuts_roster_review"} <= set(device.KERNELS)


@pytest.mark.parametrize("bad", [-1, device.MAX_REVIEW_ROOMS + 1, 1.0, "3", None, True])
def test_review_rooms_must_be_an_int_in_range(no_library, bad):
    with pytest.raises(ValueError, match="review_rooms"):
        device.Roster(4, review_rooms=bad)


def test_review_rooms_in_range_do_not_touch_the_device(no_library):
    assert device.Roster(4).review_rooms == 0
    assert device.Roster(4, review_rooms=0).review_rooms == 0
    assert device.Roster(4, review_rooms=device.MAX_REVIEW_ROOMS).review_rooms == device.MAX_REVIEW_ROOMS >= 1024
    device.Roster(4, review_rooms=3).clear_review([0, 2, 2])
    device.Roster(4, review_rooms=3).clear_review(1)


@pytest.mark.parametrize("record", [[True], [True, False, True, False], "yes", 1, [1, 0, 1], [True, None, False], 2.0])
def test_record_of_the_wrong_length_or_type(no_library, record):
    with pytest.raises(ValueError, match="record"):
        device.Roster(4, review_rooms=2).plan_many([GOOD, GOOD, GOOD], record=record)


@pytest.mark.parametrize("rm", [None, 2, 77])
@pytest.mark.parametrize("record", [True, [False, True, False]])
def test_a_recorded_broadcast_needs_a_ring_room(no_library, rm, record):
    with pytest.raises(ValueError, match=r"^broadcast 1: .*review ring"):
        device.Roster(4, review_rooms=2).plan_many([GOOD, (b"x\n", rm, None, 0, SAY), GOOD], record=record)


def test_a_roster_without_rings_records_nothing(no_library):
    with pytest.raises(ValueError, match=r"^broadcast 0: .*no review rings"):
        device.Roster(4).plan_many([GOOD], record=True)
    with pytest.raises(ValueError, match=r"^broadcast 2: .*no review rings"):
        device.Roster(4).plan_many([GOOD, GOOD, GOOD], record=[False, False, True])
    with pytest.raises(ValueError, match="no review ring"):
        device.Roster(4).review_many([0])
    with pytest.raises(ValueError, match="no review ring"):
        device.Roster(4).clear_review([0])


def test_a_bad_broadcast_is_reported_as_before(no_library):
    with pytest.raises(ValueError, match=r"^broadcast 1: text contains a NUL"):
        device.Roster(4, review_rooms=2).plan_many([GOOD, (b"a\0", 0, None, 0, SAY)], record=True)


@pytest.mark.parametrize("rooms", [[], (), 3, "01", [2], [-1], [0, None], [True], [0.0], None])
def test_review_many_rejects_bad_rooms_before_the_device(no_library, rooms):
    with pytest.raises(ValueError):
        device.Roster(4, review_rooms=2).review_many(rooms)


@pytest.mark.parametrize("rooms", [[2], [-1], "0", [None], 5])
def test_clear_review_rejects_bad_rooms_and_changes_nothing(no_library, rooms):
    r = device.Roster(4, review_rooms=2)
    with pytest.raises(ValueError):
        r.clear_review(rooms)
    assert not r._clear_pending and not r._clear.any()


def test_a_closed_roster_raises(no_library):
    with device.Roster(4, review_rooms=2) as r:
        pass
    for call in (lambda: r.review_many([0]), lambda: r.clear_review([0]), lambda: r.plan_many([GOOD], record=True)):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_record_none_packs_what_no_record_packs_and_true_sets_bit_2_alone(no_library):
    r = device.Roster(8, review_rooms=4)
    calls = [(b"ab\n", 3, 7, 1, device.COM_SHOUT), ("", 0, None, 0, SAY), (b"xyz", 1, 0, True, device.COM_SEMOTE)]
    plain, none = r._prepare_plan(calls), r._prepare_plan(calls, record=None)
    some = r._prepare_plan(calls, record=[True, False, True])
    every = r._prepare_plan(calls, record=np.bool_(True))
    for i, (a, b, c, d) in enumerate(zip(plain, none, some, every)):
        assert type(a) is type(b) is type(c)
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype == c.dtype and a.tolist() == b.tolist()
            if i != 5:
                assert a.tolist() == c.tolist() == d.tolist()
        else:
            assert a == b == c == d
    assert plain[5].tolist() == [2, 0, 2] and some[5].tolist() == [6, 0, 6] and every[5].tolist() == [6, 4, 6]
    assert r._prepare_plan(calls, record=False)[5].tolist() == [2, 0, 2]


# ---------------------------------------------- the CPU model of the rings
def test_the_model_reproduces_the_references_review():
    """tests/golden/review.json up to its first .review: every line that is not a dot command is recorded as the other
    client received it ("\\n\\r" back to "\\n"); the model's colour-off review is what the reference sent between its
    header and its footer."""
    steps = json.loads((REPO / "tests" / "golden" / "review.json").read_text())["steps"]
    at = next(i for i, s in enumerate(steps) if s.get("send") == ".review")
    model, records = Rings(1), 0
    for s in steps[:at]:
        if s["op"] == "line" and not s["send"].startswith("."):
            other = "b" if s["actor"] == "a" else "a"
            model.record(0, s["recv"][other].replace("\n\r", "\n").encode("latin-1"))
            records += 1
    assert records == 19 and model.revline[0].value == 4
    got = steps[at]["recv"]["a"].encode("latin-1")
    header, footer = b"*** Review buffer for the drive ***\n\r\n\r", b"\n\r*** End ***\n\r\n\r"
    body = got[got.index(header) + len(header):got.rindex(footer)]
    assert b"".join(model.chunks(0, 0)) == body
    assert len(model.lines(0)) == 15 and model.lines(0)[0] == b"Alice says: review line 04\n"
    assert model.lines(0)[-1] == b"- echoes into the buffer\n"


def test_the_strncpy_corner_cases_of_record():
    m = Rings(1)
    for text in (b"x" * 199, b"y" * 200, b"z" * 201, b"w" * 1999, b"short\n"):
        m.record(0, text)
    assert m.lines(0) == [b"x" * 199, b"y" * 200 + b"\n", b"z" * 200 + b"\n", b"w" * 200 + b"\n", b"short\n"]
    for i in range(10):
        m.record(0, b"line %d\n" % i)
    assert len(m.lines(0)) == 15 and m.lines(0)[0] == b"x" * 199
    m.record(0, b"")                                                    # stores an empty line over the oldest one
    assert len(m.lines(0)) == 14 and m.lines(0)[0] == b"y" * 200 + b"\n" and m.revline[0].value == 1
    m.clear(0)
    assert m.lines(0) == [] and m.revline[0].value == 0 and m.chunks(0, 1) == []


# ---------------------------------------------- bounds
def worst_lines() -> list[bytes]:
    """Stored lines that could be the costliest: a line is a text cut to 200 bytes plus the forced newline, or shorter."""
    cut = lambda t: t[:200] + b"\n" if len(t) >= 200 else t
    texts = [b"\n" * 200, b"\n" * 199, b"~FR" * 67, b"~RS" * 67, b"x" + b"~FR" * 67, b"xx" + b"~FR" * 66 + b"~F",
             b"~FR" * 66 + b"~FRx", b"x" * 1999, b"x" * 200, b"~" * 200, b"/~" * 100, b"\n~FR" * 50, b"~FR\n" * 50,
             b"x" * 199 + b"~FR", b"x" * 198 + b"~FR"]
    texts += [b"x" * a + b"\n" * (200 - a) for a in range(1, 12)]        # the flush lands on every phase of the newlines
    texts += [b"x" * a + b"~FR" * ((200 - a) // 3) for a in range(0, 6)]
    return [cut(t) for t in texts]


def test_the_per_line_bounds_hold_at_the_worst_lines():
    most_bytes, most_writes = {0: 0, 1: 0}, {0: 0, 1: 0}
    for line in worst_lines():
        assert 0 < len(line) <= device.REVIEW_LEN + 1
        for c in (0, 1):
            ch = nuts_path.chunks(line, c)
            most_bytes[c] = max(most_bytes[c], sum(map(len, ch)))
            most_writes[c] = max(most_writes[c], len(ch))
    assert most_bytes == {0: 402, 1: 1210} and most_writes == {0: 1, 1: 3}
    assert [len(x) for x in nuts_path.chunks(b"\n" * 201, 1)] == [996, 210, 4]
    assert device.MAX_LINE_BYTES == 1210 == 6 * (device.REVIEW_LEN + 1) + 4 and device.MAX_LINE_WRITES == 3
    assert device.MAX_REVIEW_BYTES == 15 * 1210 == 18_150 and device.MAX_REVIEW_WRITES == 45
    # no input byte costs more than a colour newline's 6, so 6 * 201 + 4 is a bound for every line, not only these;
    # and a write before the last two carries more than 994 bytes, so 1206 body bytes are at most 2 writes, and the reset
    assert max(len(nuts_path.transduce(bytes([b]), 1)) - 4 for b in range(1, 256)) == 6


def hand_built_review():
    """A Review from the model alone: variants at scattered places of a buffer of 0xAA bytes, -7 in the unused chunk
    sizes, garbage after each stored line's NUL."""
    m = Rings(3)
    for i, t in enumerate([b"~FRred~RS\n", b"", b"x" * 250, b"\n" * 200, b"plain\n"] + [b"line %d\n" % i for i in range(14)]):
        m.record(i % 2, t)
    rooms = [1, 0, 2, 1]
    stored = np.full((4, 15, 202), 0x55, dtype=np.uint8)
    variants = np.full(80_000, 0xAA, dtype=np.uint8)
    starts, sizes = np.zeros((4, 2), dtype=np.int64), np.zeros((4, 2), dtype=np.int64)
    counts = np.zeros((4, 2), dtype=np.int32)
    wsz = np.full((4, 2, device.MAX_REVIEW_WRITES), -7, dtype=np.int32)
    at = 11
    for q, rm in enumerate(rooms):
        rev = m.revline[rm].value
        for i in range(15):
            raw = m.ring[rm].raw[((rev + i) % 15) * 202:][:202].split(b"\0", 1)[0]
            stored[q, i, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
            stored[q, i, len(raw)] = 0
        for c in (1, 0):
            ch = m.chunks(rm, c)
            data = b"".join(ch)
            starts[q, c], sizes[q, c], counts[q, c] = at, len(data), len(ch)
            variants[at:at + len(data)] = np.frombuffer(data, dtype=np.uint8)
            wsz[q, c, :len(ch)] = [len(x) for x in ch]
            at += len(data) + 3 + 5 * q
    rv = device.Review(rooms=np.array(rooms, dtype=np.int32),
                       line_counts=np.array([len(m.lines(rm)) for rm in rooms], dtype=np.int32), stored=stored,
                       variants=variants, variant_starts=starts, variant_sizes=sizes, write_counts=counts,
                       write_sizes=wsz)
    return rv, m, rooms


def test_a_hand_built_review_obeys_the_contract(no_library):
    rv, m, rooms = hand_built_review()
    for q, rm in enumerate(rooms):
        lines = rv.lines(q)
        assert lines == m.lines(rm) and len(lines) == rv.line_counts[q]
        for c in (0, 1):
            assert rv.chunks(q, c) == [x for line in lines for x in nuts_path.chunks(line, c)]
            assert rv.variant(q, c) == b"".join(rv.chunks(q, c))
        assert rv.chunks(q, 1).count(RESET) >= len(lines)               # every line ends in its own reset write
    assert rv.lines(2) == [] and rv.chunks(2, 1) == [] and rv.variant(2, 0) == b""      # nothing was said in room 2
    assert b"x" * 200 + b"\n" in rv.lines(1) and b"" not in rv.lines(0)
    assert rv.timing == {} and rv.sequential is None
    for q, c in ((4, 0), (-1, 0), (0, 2), (0, -1)):
        with pytest.raises(IndexError):
            rv.variant(q, c)
        with pytest.raises(IndexError):
            rv.chunks(q, c)
    with pytest.raises(IndexError):
        rv.lines(4)


# ---------------------------------------------- the local rule
ALPHABET = [b"~", b"~", b"/", b"\n", b"\n", b"F", b"R", b"B", b"S", b"O", b"L", b"K", b"a", b" ", b"x", b"\xe9"]


def seeded_lines(seed: int, n: int) -> list[bytes]:
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        x = rng.random()
        if x < 0.15:                                                    # newline-heavy: outputs on both sides of 994
            k = rng.randint(150, 201)
            body = [b"\n"] * k + [rng.choice(ALPHABET) for _ in range(rng.randint(0, 201 - k))]
            rng.shuffle(body)
        elif x < 0.25:
            body = [rng.choice((b"~FR", b"~RS", b"/~", b"~", b"\n", b"/", b"~B", b"~OL")) for _ in range(rng.randint(0, 67))]
        else:
            body = [rng.choice(ALPHABET) for _ in range(rng.randint(0, 201))]
        out.append(b"".join(body)[:201])
    return out


def test_the_local_rule_equals_the_transducer_up_to_994_bytes():
    lines = seeded_lines(1502, 120_000) + [t[:201] for t in special_texts() if b"\0" not in t]
    lines += [b"\n" * 165 + b"abcd", b"\n" * 165 + b"abcde", b"abcd" + b"\n" * 165, b"x" * 194 + b"~" + b"\n" * 6]
    assert len(lines) >= 100_000 and max(map(len, lines)) == 201
    wave = {0: 0, 1: 0}
    sequential = {0: 0, 1: 0}
    sizes_seen = set()
    for lo in range(0, len(lines), 10_000):
        batch = lines[lo:lo + 10_000]
        for c in (0, 1):
            flat, sizes = local_rule(batch, c)
            at = 0
            for line, n in zip(batch, sizes.tolist()):
                body, at = flat[at:at + n], at + n
                want = nuts_path.transduce(line, c)
                assert len(want) == n + 4 * c, (line, c)                # the sizes agree at any length
                if c:
                    sizes_seen.add(n)
                if n > WAVE_LIMIT:                                      # the kernel's sequential path
                    sequential[c] += 1
                    continue
                wave[c] += 1
                assert body + RESET * c == want, (line, c)
        if lo == 0:                                                     # and no flush fired: one write, then the reset
            for line in batch[:3000] + lines[-4:]:
                for c in (0, 1):
                    want = nuts_path.transduce(line, c)
                    if len(want) - 4 * c <= WAVE_LIMIT:
                        body = want[:len(want) - 4 * c]
                        assert nuts_path.chunks(line, c) == ([body] if body else []) + [RESET] * c, (line, c)
    assert sequential[0] == 0 and sequential[1] > 1000 and wave[1] > 100_000
    assert {994, 995} <= sizes_seen                                     # each side of the threshold is present
    # past the threshold a flush can fire in mid-line: the rule's bytes still agree, its single write does not
    line = b"x" * 995 + b"~"
    assert len(nuts_path.chunks(line, 1)) == 3 and nuts_path.chunks(b"\n" * 165 + b"abcd", 1)[0][-4:] == b"abcd"
    assert [len(x) for x in nuts_path.chunks(b"\n" * 166 + b"~", 1)] == [996, 1, 4]


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def review_run(built):
    res = child_run.run_child("device_review_child.py", "DEVICE_REVIEW", 600)
    print("\n[review]", json.dumps(res)[:3000])
    return res


@pytest.mark.gpu
def test_random_histories_match_the_model(review_run):
    r = review_run["random"]
    assert [rr for rr, _ in r["rosters"]] == [1, 2, 15, 16, device.MAX_REVIEW_ROOMS]
    assert {1, 1000} <= {cap for _, cap in r["rosters"]}
    assert r["ks"] == [1, 7, 100, 1000] and r["record_modes"] == ["all", "mix", "none"]
    assert r["calls"] >= 20 and r["reviews"] >= 5 and r["updates"] > 0 and r["clears"] > 0 and r["fanouts"] > 0
    assert r["most_records_into_one_room_in_one_call"] > 15 and r["duplicate_rooms_reviewed"] > 0
    assert r["rooms_reviewed"] > 1000 and r["lines_compared"] > 0
    assert r["sequential_lines"] > 0 and r["wave_lines"] > 0
    assert r["n_bad"] == 0, r["first_bad"]


@pytest.mark.gpu
def test_every_special_text_is_recorded_and_reviewed(review_run):
    s = review_run["specials"]
    assert s["texts"] >= 314 + 20 and s["lines_compared"] >= s["texts"] - 1      # the empty text stores no line
    assert s["sequential_lines"] > 0 and s["wave_lines"] > 600
    assert s["n_bad"] == 0, s["first_bad"]


@pytest.mark.gpu
def test_plans_with_record_equal_their_twins_without(review_run):
    assert review_run["random"]["n_bad_plan"] == 0
    p = review_run["copies"]["plan"]
    assert p["with_rings"]["dirty"] == p["without_rings"]["dirty"]
    assert p["with_rings"]["clean"] == p["without_rings"]["clean"]
    assert p["with_rings"]["clean"][0] < p["with_rings"]["dirty"][0]
    assert p["with_rings"]["recording"] == p["with_rings"]["clean"]     # no clear was pending: not a byte more
    assert p["with_rings"]["clean_after_recording"] == p["with_rings"]["clean"]


@pytest.mark.gpu
def test_order_of_records_clears_and_reviews(review_run):
    o = review_run["order"]
    assert o["line_counts"] == [14, 13, 14, 0]           # 42 texts over three rooms; room 1 holds the empty one
    for key in ("one_call_equals_k_calls", "cleared_room_is_empty", "other_rooms_kept", "clear_then_record",
                "room_2_still_kept", "earlier_review_unchanged", "later_review_differs"):
        assert o[key] is True, (key, o)


@pytest.mark.gpu
def test_copy_volume_of_review_many_depends_on_q_alone(review_run):
    c = review_run["copies"]["review"]
    stride = (15 * device.MAX_LINE_BYTES + 3) & ~3
    for q in (1, 5, 64):
        v = c[str(q)]
        assert v["full"] == v["empty"], v                               # not on what the rings hold
        assert v["empty_bytes"] == 0 and v["full_bytes"] == q * 15 * (402 + 1210)
        h2d, d2h = v["full"]
        assert 0 < h2d <= 4 * q + 4 + 2 * 256
        per_room = 2 * stride + 15 * 202 + 4 * (2 * device.MAX_REVIEW_WRITES + 2 + 2 + 1 + 1)
        assert q * 2 * 15 * device.MAX_LINE_BYTES <= d2h <= q * per_room + 4 + 8 * 256, (v, per_room)
    assert c["1"]["full"] < c["5"]["full"] < c["64"]["full"]
