"""``Roster.speak_many``: say(), shout(), emote() and semote() composed on the device (nuts_roster_speak and
nuts_roster_speak_plan of fanout.hip), ``device.Speech``, and the speaker fields of ``Roster.update``.

Host tier (unmarked): everything malformed is rejected before the device library loads, and a rejected update changes
nothing; the Python model of the command functions (``model`` of tests/device_speak_child.py, built from
``np_say_verb`` / ``np_contains_swearing`` and the reference's format strings) reproduces what every client received in
four recorded sessions of tests/golden, 86 comparisons; the notices occur in tests/golden/errors.json; a composed text
is at most ``len(inpstr) + 32`` bytes and its transduced variants stay within ``max_bytes`` and ``MAX_WRITES``; the
kernel's swear scan, stated in numpy with its slices and overlap, equals ``np_contains_swearing`` on more than 100,000
seeded strings; a ``Speech`` built by hand obeys its contract.  The kernels' scratch-free compile is
tests/test_device_fanout.py's, over every name in ``device.KERNELS``.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_speak_child.py, under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import json
import random
from pathlib import Path

import numpy as np
import pytest

import child_run
from device_speak_child import (CAPACITIES, COMS, EMOTE, EVENTS_PER_CALL, GOLDEN, GOLDEN_COMPARISONS, MUZZLED_NOTICE,
                                NOSWEARING, SAY, SEMOTE, SHOUT, SWEAR_WORDS, WHAT_NOTICE, model, model_answer, replay,
                                swear_rule)
from nuts333_amd import device, nuts_path

REPO = Path(__file__).resolve().parent.parent


def seated(capacity=4, review_rooms=0) -> device.Roster:
    """A roster whose slots 0 and 1 can speak: a room and a name."""
    r = device.Roster(capacity, review_rooms=review_rooms)
    r.update([0, 1], room=0, name=[b"Alice", "Bobby"])
    return r


GOOD = (0, SAY, b"hello there", 2)


# ------------------------------------------------------------------ host tier: input checks
@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


def test_the_new_names_exist():
    assert {"nuts_roster_speak", "nuts_roster_speak_plan"} <= set(device.KERNELS)
    assert (device.COM_SAY, device.COM_SHOUT, device.COM_EMOTE, device.COM_SEMOTE) == (3, 4, 6, 7)
    assert (device.SPOKEN, device.MUZZLED, device.NOTHING, device.SWEARING) == (0, 1, 2, 3)
    assert device.INVISNAME == b"A presence" and device.USER_NAME_LEN == 12 and device.ARR_SIZE == 1000


@pytest.mark.parametrize("events", [[], (), None, 3, "say", b"say", np.zeros(3)])
def test_events_must_be_a_non_empty_sequence(no_library, events):
    with pytest.raises(ValueError, match="events|empty call"):
        seated().speak_many(events)


@pytest.mark.parametrize("bad, why", [
    ([0, SAY, b"x", 2], "tuple"), ((0, SAY, b"x"), "tuple"), ((0, SAY, b"x", 2, 0), "tuple"),
    ((4, SAY, b"x", 2), "slot"), ((-1, SAY, b"x", 2), "slot"), ((None, SAY, b"x", 2), "slot"), ((True, SAY, b"x", 2), "slot"),
    ((0, 5, b"x", 2), "com"), ((0, 0, b"x", 2), "com"), ((0, "say", b"x", 2), "com"), ((0, True, b"x", 2), "com"),
    ((0, 3.0, b"x", 2), "com"), ((0, SAY, b"a\0b", 2), "NUL"), ((0, SAY, 5, 2), "text must be"),
    ((0, SAY, "Ā", 2), "outside one byte"), ((0, SAY, b"x" * 1000, 2), "at most 999"),
    ((0, SHOUT, "y" * 1999, 2), "at most 999"), ((0, SAY, b"x", -1), "word_count"), ((0, SAY, b"x", 11), "word_count"),
    ((0, SAY, b"x", 1.0), "word_count"), ((0, SAY, b"x", None), "word_count"), ((0, SAY, b"x", True), "word_count"),
])
def test_a_malformed_event_is_rejected_by_its_number(no_library, bad, why):
    with pytest.raises(ValueError, match=rf"^event 1: .*{why}"):
        seated().speak_many([GOOD, bad, GOOD])


def test_the_longest_inpstr_and_every_word_count_pass_the_checks(no_library):
    r = seated()
    for com in COMS:
        packed = r._prepare_speech([(1, com, b"x" * 999, wc) for wc in range(11)] + [(0, com, "", 0)], False, False)
        assert packed[2].tolist() == [999] * 11 + [0] and packed[5].tolist() == list(range(11)) + [0]
        assert packed[3].tolist() == [1] * 11 + [0] and set(packed[4].tolist()) == {com}


@pytest.mark.parametrize("flag", ["ban_swearing", "record"])
@pytest.mark.parametrize("bad", [2, -1, None, "yes", 1.0, [True]])
def test_the_call_flags_must_be_bools(no_library, flag, bad):
    with pytest.raises(ValueError, match=flag):
        seated(review_rooms=1).speak_many([GOOD], **{flag: bad})


def test_the_speaker_needs_a_room_a_name_and_no_login(no_library):
    r = seated()
    r.update(2, name=b"Carol")                           # no room
    r.update(3, room=0)                                  # no name
    with pytest.raises(ValueError, match=r"^event 1: .*slot 2, has no room"):
        r.speak_many([GOOD, (2, SAY, b"x", 2)])
    with pytest.raises(ValueError, match=r"^event 0: .*slot 3, has no name"):
        r.speak_many([(3, EMOTE, b";x", 1)])
    r.update(1, login=1)
    with pytest.raises(ValueError, match=r"^event 2: .*slot 1, is still logging in"):
        r.speak_many([GOOD, GOOD, (1, SHOUT, b"x", 2)])
    r.update(0, room=None)
    with pytest.raises(ValueError, match=r"^event 0: .*no room"):
        r.speak_many([GOOD])


def test_a_recorded_say_or_emote_needs_a_ring_room_whatever_its_outcome(no_library):
    r = seated(review_rooms=2)
    r.update(1, room=2, muzzled=1)
    for com in (SAY, EMOTE):
        with pytest.raises(ValueError, match=r"^event 1: .*room 2 has no review ring"):
            r.speak_many([GOOD, (1, com, b"never said", 2)], record=True)
    with pytest.raises(ValueError, match=r"^event 0: .*no review ring.*review_rooms is 0"):
        seated().speak_many([GOOD], record=True)
    # shouts and semotes are never recorded, so their speakers may stand anywhere: these pass the checks
    for r2 in (r, seated()):
        packed = r2._prepare_speech([(1, SHOUT, b"x y", 2), (1, SEMOTE, b"#x", 1)], False, True)
        assert packed[-1] is False
    assert r._prepare_speech([(1, SHOUT, b"x y", 2), GOOD], True, True)[-2:] == (1, True)


def test_a_closed_roster_raises(no_library):
    with seated() as r:
        pass
    with pytest.raises(ValueError, match="closed"):
        r.speak_many([GOOD])
    with pytest.raises(ValueError, match="closed"):
        r.update(0, name=b"x")


@pytest.mark.parametrize("fields", [
    {"name": b""}, {"name": b"x" * 13}, {"name": b"a\0b"}, {"name": 5}, {"name": None}, {"name": "Ā"},
    {"name": [b"ok"]}, {"name": [b"ok", b"fine", b"three"]}, {"name": [b"ok", b""]}, {"vis": 2}, {"vis": "1"},
    {"muzzled": -1}, {"muzzled": [0]}, {"command_mode": None}, {"command_mode": [1, 2]},
    {"name": b"fine", "vis": 1, "muzzled": 0, "command_mode": 7}, {"name": b"fine", "room": -4},
    {"muzzled": 1, "colour": 3},
])
def test_a_rejected_update_changes_nothing(no_library, fields):
    r = seated()
    r.update([0, 1], vis=[1, 0], muzzled=[0, 1], command_mode=1)
    r._dirty = r._speech_dirty = False
    table, speech = r._table.copy(), r._speech.copy()
    with pytest.raises(ValueError):
        r.update([0, 1], **fields)
    assert np.array_equal(r._table, table) and np.array_equal(r._speech, speech)
    assert r._dirty is False and r._speech_dirty is False


def test_the_speech_mirror_and_its_dirty_flag(no_library):
    r = device.Roster(5)
    assert r._speech.shape == (5, 16) and r._speech.dtype == np.uint8 and r._speech_dirty
    assert r._speech[:, 13].tolist() == [1] * 5 and not r._speech[:, :13].any()      # visible, nameless
    r._dirty = r._speech_dirty = False
    r.update([1, 3, 1], name=[b"First", "Abcdefghijkl", b"Last"], vis=0, muzzled=[1, 0, 0], command_mode=[0, 1, 1])
    assert r._dirty is False and r._speech_dirty is True                # a speech-only update leaves _dirty as it was
    assert r._speech[1].tobytes() == b"Last" + b"\0" * 8 + bytes([4, 4, 0, 0])       # the last values win
    assert r._speech[3].tobytes() == b"Abcdefghijkl" + bytes([12, 4, 0, 0])
    assert r._speech[0].tobytes() == b"\0" * 13 + bytes([1, 0, 0])
    r.update(1, name=b"Al", vis=True, muzzled=np.bool_(True))
    assert r._speech[1].tobytes() == b"Al" + b"\0" * 10 + bytes([2, 7, 0, 0])
    r._speech_dirty = False
    r.update(2, room=3)                                                 # and a table-only update leaves _speech_dirty
    assert r._dirty is True and r._speech_dirty is False
    r._dirty = False
    r.update(2, colour=1, muzzled=1)                                    # both kinds of field: both mirrors
    assert r._dirty is True and r._speech_dirty is True
    assert r._table.nbytes == 5 * 5                                     # the 5-byte-per-slot table is what it was


# ---------------------------------------------- the model is the reference
@pytest.mark.parametrize("name", GOLDEN)
def test_the_model_reproduces_what_every_client_received(name):
    res = replay(name, model_answer)
    assert res["mismatches"] == []
    assert res["comparisons"] == GOLDEN_COMPARISONS[name]               # it cannot pass by skipping
    assert sum(GOLDEN_COMPARISONS.values()) == 86


def test_semote_has_no_swear_check_and_the_others_do():
    steps = json.loads((REPO / "tests" / "golden" / "swearing.json").read_text())["steps"]
    by_send = {s.get("send"): s["recv"] for s in steps}
    assert by_send["#shit is allowed in semotes"]["b"] == "!! Aliceshit is allowed in semotes\n\r"
    assert by_send[";says cunt"] == {"a": "Swearing is not allowed here.\n\r"}
    alice = {"slot": 0, "room": 0, "name": b"Alice", "vis": 1, "muzzled": 0, "command_mode": 0}
    assert model(alice, SEMOTE, b"#shit is allowed in semotes", 5, True)["outcome"] == device.SPOKEN
    for com, text in ((SAY, b"what the FuCk"), (SHOUT, b"oh shit"), (EMOTE, b";says cunt"), (SAY, b"scunthorpe problem")):
        m = model(alice, com, text, 3, True)
        assert m["outcome"] == device.SWEARING and m["reply"] == NOSWEARING and m["line"] is None
        assert model(alice, com, text, 3, False)["outcome"] == device.SPOKEN


def test_the_notices_occur_in_the_recorded_errors():
    steps = json.loads((REPO / "tests" / "golden" / "errors.json").read_text())["steps"]
    seen = {text for s in steps for text in s.get("recv", {}).values()}
    for notice in set(WHAT_NOTICE.values()) | set(MUZZLED_NOTICE.values()):
        wire = notice.decode().replace("\n", "\n\r")
        assert any(text == wire or text.startswith(wire) for text in seen), notice
    assert len(set(WHAT_NOTICE.values())) == 4 and len(set(MUZZLED_NOTICE.values())) == 3


def test_the_outcome_order_and_the_stale_byte_rule():
    sp = {"slot": 0, "room": 0, "name": b"Al", "vis": 1, "muzzled": 1, "command_mode": 1}
    assert model(sp, SAY, b"shit", 1, True)["outcome"] == device.MUZZLED         # muzzled before everything
    sp["muzzled"] = 0
    assert model(sp, SAY, b"shit", 1, True)["outcome"] == device.NOTHING         # then "Say what?"
    assert model(sp, SAY, b"shit", 2, True)["outcome"] == device.SWEARING
    sp["command_mode"] = 0
    assert model(sp, SAY, b"", 0, False)["line"] == b"Al says: \n"               # speech mode says an empty line
    for com, lead in ((EMOTE, b";"), (SEMOTE, b"#")):
        assert model(sp, com, lead, 1, False)["outcome"] == device.NOTHING       # byte 1 past the end counts as 0
        assert model(sp, com, b"", 0, False)["outcome"] == device.NOTHING
        assert model(sp, com, lead + b" x", 1, False)["outcome"] == device.NOTHING
        assert model(sp, com, lead + b"\xe9", 1, False)["outcome"] == device.NOTHING   # a signed char: 0xe9 < 33
        assert model(sp, com, lead + b"x", 1, False)["outcome"] == device.SPOKEN
        assert model(sp, com, lead, 2, False)["outcome"] == device.SPOKEN


# ---------------------------------------------- bounds
def test_a_composed_text_is_at_most_32_bytes_longer_than_inpstr():
    texts = [b"", b"x", b"?", b"!", b";", b"#", b";x", b"#x", b"hello there!", b"x" * 999, b"\n" * 998 + b"!"]
    most = 0
    for name, vis in ((b"Abcdefghijkl", 1), (b"Abcdefghijkl", 0), (b"A", 1), (b"A", 0)):
        sp = {"slot": 0, "room": 0, "name": name, "vis": vis, "muzzled": 0, "command_mode": 0}
        for com in COMS:
            for t in texts:
                m = model(sp, com, t, 5, False)
                assert m["outcome"] == device.SPOKEN
                for composed in (m["line"], m["reply"]):
                    if composed is not None:
                        assert len(composed) <= len(t) + device.COMPOSED_EXTRA == len(t) + 32
                        most = max(most, len(composed) - len(t))
    assert most == len(b"~OLAbcdefghijkl shouts:~RS \n") == 28
    # the notices are not composed from inpstr; the longest is what a text slot's extra width has to hold
    notices = [*WHAT_NOTICE.values(), *MUZZLED_NOTICE.values(), NOSWEARING]
    assert max(map(len, notices)) == 35 <= device._SPEAK_SLACK and device.COMPOSED_EXTRA <= device._SPEAK_SLACK


def test_the_worst_inpstr_stays_within_the_variant_bounds():
    sp = {"slot": 0, "room": 0, "name": b"Abcdefghijkl", "vis": 1, "muzzled": 0, "command_mode": 0}
    for t in (b"\n" * 999, b"\n" * 998 + b"!", b"~FR" * 333, b";" + b"\n" * 998):
        for com in COMS:
            m = model(sp, com, t, 5, False)
            for composed in (m["line"], m["reply"]):
                if composed is None:
                    continue
                assert len(composed) < device.TEXT_SIZE
                for c in (0, 1):
                    ch = nuts_path.chunks(composed, c)
                    assert sum(map(len, ch)) <= device.max_bytes(len(composed)) and len(ch) <= device.MAX_WRITES
    line = model(sp, SAY, b"\n" * 999, 5, False)["line"]
    assert len(nuts_path.transduce(line, 1)) == 6 * 1000 + len(b"Abcdefghijkl says: ") + 4


# ---------------------------------------------- the kernel's swear rule
def swear_strings(seed: int, n: int) -> list[bytes]:
    rng = random.Random(seed)
    out = []
    filler = lambda k: bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz  FSCUHIKNT\xe9\xc6\x80\xff~\n") for _ in range(k))
    for _ in range(n):
        x = rng.random()
        length = rng.choice((rng.randrange(0, 40), rng.randrange(0, 1000), 999))
        if x < 0.3:
            t = filler(length)
        else:
            w = bytes(rng.choice((ch, ch ^ 32)) for ch in rng.choice(SWEAR_WORDS))          # mixed case
            if x < 0.5:                                                                      # a near miss
                w = rng.choice((w[:3], w[1:], w[:2] + b" " + w[2:], w[:3] + bytes([w[3] | 0x80]),
                                bytes([w[0] | 0x80]) + w[1:], w[:1] + w[2:], w[:3] + b"\0"[:0] + w[:3]))
            length = max(length, len(w))
            at = rng.choice((0, length - len(w), rng.randrange(length - len(w) + 1)))      # first, last, anywhere
            t = filler(at) + w + filler(length - len(w) - at)
        out.append(t[:999])
    # a word straddling every slice boundary, by every amount, and ending exactly at byte 999
    for boundary in range(16, 999, 16):
        for back in range(0, 5):
            w = SWEAR_WORDS[(boundary + back) % 3]
            w = w.upper() if boundary % 32 else w
            out.append(b"x" * (boundary - back) + w + b"y" * rng.randrange(3))
            out.append(b"x" * (boundary - back) + w[:3])
    out += [b"x" * 995 + w for w in SWEAR_WORDS] + [w for w in SWEAR_WORDS] + [b"", b"f", b"fuc", b"FUCK", b"sHiT!"]
    return out


def test_the_kernels_swear_rule_equals_the_restatement():
    texts = swear_strings(1703, 100_000)
    assert len(texts) >= 100_000 and max(map(len, texts)) == 999
    lib = nuts_path.lib()
    hits = misses = 0
    for lo in range(0, len(texts), 5000):
        batch = texts[lo:lo + 5000]
        got = swear_rule(batch)
        for t, g in zip(batch, got.tolist()):
            want = bool(lib.np_contains_swearing(t))
            assert g == want, t
            hits += want
            misses += not want
    assert hits > 30_000 and misses > 30_000
    assert any(b >= 0x80 for t in texts[:1000] for b in t)


# ---------------------------------------------- the dataclass
def hand_built_speech():
    """A Speech from the model alone, for a 70-slot roster: texts and variants scattered over buffers of 0xAA bytes, -7
    in the unused chunk sizes."""
    cap, words = 70, 2
    speakers = {5: {"slot": 5, "room": 0, "name": b"Five", "vis": 1, "muzzled": 0, "command_mode": 1},
                66: {"slot": 66, "room": 1, "name": b"Sixtysix", "vis": 0, "muzzled": 0, "command_mode": 0},
                9: {"slot": 9, "room": 0, "name": b"Nine", "vis": 1, "muzzled": 1, "command_mode": 0}}
    events = [(5, SAY, b"~FRred~RS hello?", 2), (5, SAY, b"", 0), (66, SHOUT, b"loud\n\n!", 2), (66, EMOTE, b";waves", 1),
              (5, SEMOTE, b"#s", 1), (9, SAY, b"mmph", 1), (66, SHOUT, b"", 1), (5, EMOTE, b"is shit", 2)]
    colour = np.arange(cap) % 3 == 0
    k = len(events)
    texts = np.full(4000, 0xAA, dtype=np.uint8)
    variants = np.full(40_000, 0xAA, dtype=np.uint8)
    tstarts, tsizes = np.zeros((2, k), dtype=np.int64), np.full((2, k), -1, dtype=np.int64)
    starts, sizes = np.zeros((2, k, 2), dtype=np.int64), np.zeros((2, k, 2), dtype=np.int64)
    counts = np.zeros((2, k, 2), dtype=np.int32)
    wsz = np.full((2, k, 2, device.MAX_WRITES), -7, dtype=np.int32)
    bits = np.zeros((2, k, words), dtype=np.uint64)
    outcome = np.zeros(k, dtype=np.int8)
    models, at, vat = [], 3, 7
    for j, (slot, com, inpstr, wc) in enumerate(events):
        m = model(speakers[slot], com, inpstr, wc, True)
        models.append(m)
        outcome[j] = m["outcome"]
        for row, text in enumerate((m["line"], m["reply"])):
            if text is None:
                continue
            tstarts[row, j], tsizes[row, j] = at, len(text)
            texts[at:at + len(text)] = np.frombuffer(text, dtype=np.uint8)
            at += len(text) + 5
            for c in (0, 1):
                ch = nuts_path.chunks(text, c)
                data = b"".join(ch)
                starts[row, j, c], sizes[row, j, c], counts[row, j, c] = vat, len(data), len(ch)
                variants[vat:vat + len(data)] = np.frombuffer(data, dtype=np.uint8)
                wsz[row, j, c, :len(ch)] = [len(x) for x in ch]
                vat += len(data) + 3
        if m["line"] is not None:                        # everyone else in a room hears it
            admitted = np.ones(cap, dtype=bool)
            if m["sender"] is not None:
                admitted[m["sender"]] = False
            bits[0, j] = device._pack(admitted)
        if m["reply"] is not None:
            bits[1, j, slot // 64] = np.uint64(1) << np.uint64(slot % 64)
    plans = [device.Plan(capacity=cap, admitted_bits=bits[i], colour_bits=device._pack(colour), variants=variants,
                         variant_starts=starts[i], variant_sizes=sizes[i], write_counts=counts[i], write_sizes=wsz[i])
             for i in (0, 1)]
    sp = device.Speech(outcome=outcome, room=plans[0], reply=plans[1], texts=texts, text_starts=tstarts,
                       text_sizes=tsizes)
    return sp, events, models, colour


def test_a_hand_built_speech_obeys_the_contract(no_library):
    sp, events, models, colour = hand_built_speech()
    assert sp.outcome.tolist() == [0, 2, 0, 0, 0, 1, 2, 3] and sp.timing == {}
    for k, ((slot, com, inpstr, wc), m) in enumerate(zip(events, models)):
        assert sp.line(k) == (m["line"] or b"") and sp.reply_text(k) == (m["reply"] or b"")
        for plan, text in ((sp.room, m["line"]), (sp.reply, m["reply"])):
            for c in (0, 1):
                assert plan.chunks(k, c) == (nuts_path.chunks(text, c) if text is not None else [])
                assert plan.variant(k, c) == b"".join(plan.chunks(k, c))
        assert sp.reply.admitted(k).nonzero()[0].tolist() == ([slot] if m["reply"] is not None else [])
        if m["line"] is None:
            assert not sp.room.admitted(k).any() and not sp.room.variant_sizes[k].any() and not sp.room.write_counts[k].any()
    assert sp.reply_text(3) == b"" and not sp.reply.variant_sizes[3].any()       # a spoken emote has no reply at all
    assert sp.line(3) == b"A presencewaves\n" and sp.line(0) == b"Five asks: ~FRred~RS hello?\n"
    assert sp.reply_text(2) == b"~OLYou shout:~RS loud\n\n!\n"
    # both plans expand into ordinary fan-outs
    room, reply = sp.room.expand(), sp.reply.expand()
    cap, k = sp.room.capacity, len(events)
    assert room.admitted.sum() == 69 + 69 + 70 + 70 and len(room.admitted) == k * cap
    assert reply.admitted.nonzero()[0].tolist() == [kk * cap + e[0] for kk, (e, m) in enumerate(zip(events, models))
                                                    if m["reply"] is not None]
    for kk, (slot, *_rest) in enumerate(events):
        i = reply.item(kk, slot)
        want = nuts_path.transduce(models[kk]["reply"], int(colour[slot])) if models[kk]["reply"] is not None else b""
        assert reply.output(i) == want
    assert room.output(room.item(0, 6)) == nuts_path.transduce(models[0]["line"], 1)
    assert room.output(room.item(0, 5)) == b"" and room.output(room.item(0, 7)) == nuts_path.transduce(models[0]["line"], 0)
    for bad_k in (-1, 8):
        with pytest.raises(IndexError):
            sp.line(bad_k)
        with pytest.raises(IndexError):
            sp.reply_text(bad_k)


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def speak_run(built):
    res = child_run.run_child("device_speak_child.py", "DEVICE_SPEAK", 600)
    print("\n[speak]", json.dumps(res)[:4000])
    return res


@pytest.mark.gpu
def test_the_golden_sessions_replay_on_the_device(speak_run):
    g = speak_run["golden"]
    assert list(g) == list(GOLDEN)
    for name in GOLDEN:
        assert g[name]["comparisons"] == GOLDEN_COMPARISONS[name], name
        assert g[name]["mismatches"] == [] and g[name]["n_bad_vs_model"] == 0, (name, g[name])
    assert sum(g[name]["comparisons"] for name in GOLDEN) == 86


@pytest.mark.gpu
def test_seeded_events_match_the_model(speak_run):
    f = speak_run["fuzz"]
    assert f["capacities"] == list(CAPACITIES) == [1, 63, 64, 65, 300, 1000]
    assert f["calls"] == 2 * len(CAPACITIES) and f["events"] == f["calls"] * EVENTS_PER_CALL and EVENTS_PER_CALL >= 200
    assert f["longest_inpstr"] == 999
    by = f["outcome_by_com"]
    for outcome in (device.SPOKEN, device.MUZZLED, device.NOTHING, device.SWEARING):
        for com in COMS:
            if (outcome, com) == (device.SWEARING, SEMOTE):
                assert f"{outcome}/{com}" not in by                     # semote has no swear check
            else:
                assert by.get(f"{outcome}/{com}", 0) > 0, (outcome, com, by)
    assert f["n_bad"] == 0, f["first_bad"]


@pytest.mark.gpu
def test_the_room_plan_is_plan_many_of_the_composed_line(speak_run):
    c = speak_run["contract"]
    assert c["checked"] >= 40 and c["coms"] == sorted(COMS)
    assert c["n_bad"] == 0, c["first_bad"]


@pytest.mark.gpu
def test_recording_says_and_emotes_into_the_rings(speak_run):
    r = speak_run["recording"]
    assert r["speak_calls"] >= 10 and r["plan_calls"] >= 3 and r["clears"] >= 3 and r["reviews"] >= 5
    assert r["recorded"] > 100 and r["lines_compared"] > 100 and r["most_into_one_room_in_one_call"] > 15
    assert all(n > 0 for n in r["not_recorded"].values()), r["not_recorded"]
    assert r["n_bad"] == 0, r["first_bad"]


@pytest.mark.gpu
def test_nothing_else_moved(speak_run):
    m = speak_run["moved"]
    for later in ("after_speaking", "after_speech_update", "after_speaking_again"):
        assert m[later] == m["before"], later                           # results and copy volumes alike
    assert m["speech_update_left_dirty"] == [False, False]
    h = m["speak_h2d"]
    cap = m["capacity"]
    assert len(set(h["clean"])) == 1 and len(m["speak_d2h"]) == 1       # the copies depend on the events alone
    assert 16 * cap <= h["after_speech_update"] - h["clean"][0] < 16 * cap + 256          # the speaker table alone
    # the table alone, in its two 256-byte aligned slices: the speaker table behind it was not given and does not travel
    assert 5 * cap <= h["after_table_update"] - h["clean"][0] < 5 * cap + 512 < 16 * cap
