"""``Roster.input_many``: client reads framed and dispatched on the device (nuts_roster_parse of fanout.hip) in front of
the speech commands, ``device.Input``, and the ``level`` field of ``Roster.update``.

Host tier (unmarked): everything malformed is rejected by read number before the device library loads, and a rejected
update changes nothing; ``level`` lands in byte 14 of the speaker record; the command table of fanout.hip is the
restatement's; the Python model of ``user_input()`` / ``exec_com()`` (``dispatch`` of tests/device_input_child.py, built
from ``np_terminate``, ``np_wordfind``, ``np_remove_first``, ``np_command_lookup`` and ``np_command_level``) replaces the
hand-written ``classify`` in the replay of the four recorded sessions ``speak_many`` is pinned on, with the same 86
comparisons, and tells the ``Unknown command.`` steps of tests/golden/errors.json from the others exactly; the kernel's
rules, stated in numpy with its lane slices, its carry between lanes, the modulo 39 and two table entries per lane,
equal the ``np_*`` functions on more than 100,000 seeded reads; an ``Input`` built by hand obeys its accessors.  The
kernel's scratch-free compile is tests/test_device_fanout.py's, over every name in ``device.KERNELS``.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_input_child.py, under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import json
import random
import re
from pathlib import Path

import numpy as np
import pytest

import child_run
from device_input_child import (CAPACITIES, COMMAND, EMPTY, IAC, KINDS, READS_PER_CALL, REPEAT, SPEECH, UNKNOWN,
                                UNKNOWN_NOTICE, answer_of, command_table, dispatch, fuzz_read, model_answer, parse_rule,
                                replay_reads, systematic_reads)
from device_speak_child import COMS, EMOTE, GOLDEN, GOLDEN_COMPARISONS, SAY, SEMOTE, SHOUT, WHAT_NOTICE
from nuts333_amd import device, nuts_path

REPO = Path(__file__).resolve().parent.parent


def seated(capacity=4, review_rooms=0) -> device.Roster:
    """A roster whose slots 0 and 1 can speak: a room and a name."""
    r = device.Roster(capacity, review_rooms=review_rooms)
    r.update([0, 1], room=0, name=[b"Alice", "Bobby"])
    return r


GOOD = (0, b"hello there\n")


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


# ------------------------------------------------------------------ host tier: input checks
def test_the_new_names_exist():
    assert "nuts_roster_parse" in device.KERNELS
    assert (device.IAC, device.EMPTY, device.REPEAT, device.UNKNOWN, device.SPEECH, device.COMMAND) == (0, 1, 2, 3, 4, 5)
    assert device.NOT_SPEECH == -1 and device.READ_SIZE == 1000 and device.MAX_LEVEL == 4
    assert callable(device.Roster.input_many) and device.Input.__dataclass_fields__.keys() >= {
        "kind", "com", "word_count", "line_sizes", "inpstr_starts", "inpstr_sizes", "speech", "timing"}
    source = device.SOURCE.read_text()
    assert re.search(r'extern "C" __global__ void __launch_bounds__\(kBlock\) nuts_roster_parse\(', source)
    assert "nd_roster_input(" in source


@pytest.mark.parametrize("reads", [[], (), None, 3, "say", b"say\n", np.zeros(3)])
def test_reads_must_be_a_non_empty_sequence(no_library, reads):
    with pytest.raises(ValueError, match="reads|empty call"):
        seated().input_many(reads)


@pytest.mark.parametrize("bad, why", [
    ([0, b"x\n"], "tuple"), ((0,), "tuple"), ((0, b"x\n", 2), "tuple"), (b"x\n", "tuple"),
    ((4, b"x\n"), "slot"), ((-1, b"x\n"), "slot"), ((None, b"x\n"), "slot"), ((True, b"x\n"), "slot"), ((0.0, b"x\n"), "slot"),
    ((0, b""), "0 bytes"), ((0, ""), "0 bytes"), ((0, b"x" * 1000 + b"\n"), "1001 bytes"),
    ((0, b"x"), "does not end a line.*get_charclient_line"), ((0, b"hello"), "does not end a line"),
    ((0, b"hi\n "), "does not end a line"), ((0, b"x\x7f"), "does not end a line"), ((0, "no newline"), "does not end a line"),
    ((0, "Ā\n"), "outside one byte"), ((0, 5), "data must be"), ((0, None), "data must be"), ((0, [10]), "data must be"),
])
def test_a_malformed_read_is_rejected_by_its_number(no_library, bad, why):
    with pytest.raises(ValueError, match=rf"^read 1: .*{why}"):
        seated().input_many([GOOD, bad, GOOD])


def test_every_byte_value_and_every_line_ending_pass_the_checks(no_library):
    r = seated()
    ends = [bytes([b]) for b in list(range(32)) + list(range(128, 256))]
    reads = [(1, b"x" * 999 + e) for e in ends] + [(0, e) for e in ends]
    reads += [(0, bytes(range(256)) + b"\n"), (0, bytearray(b"a\0b\n")), (0, memoryview(b"mv\r\n")), (1, "caf\xe9\n")]
    datas, data, off, lens, slots, ban, record = r._prepare_input(reads, False, False)
    assert len(datas) == len(reads) and data == b"".join(datas) and datas[-1] == b"caf\xe9\n"
    assert lens.tolist() == [len(d) for d in datas] and off.tolist() == np.cumsum([0] + lens.tolist())[:-1].tolist()
    assert slots.tolist() == [s for s, _ in reads] and (ban, record) == (0, 0)
    assert all(isinstance(d, bytes) for d in datas)


@pytest.mark.parametrize("flag", ["ban_swearing", "record"])
@pytest.mark.parametrize("bad", [2, -1, None, "yes", 1.0, [True]])
def test_the_call_flags_must_be_bools(no_library, flag, bad):
    with pytest.raises(ValueError, match=flag):
        seated(review_rooms=1).input_many([GOOD], **{flag: bad})


def test_the_speaker_needs_a_room_a_name_and_no_login(no_library):
    r = seated()
    r.update(2, name=b"Carol")                           # no room
    r.update(3, room=0)                                  # no name
    with pytest.raises(ValueError, match=r"^read 1: .*slot 2, has no room"):
        r.input_many([GOOD, (2, b"x\n")])
    with pytest.raises(ValueError, match=r"^read 0: .*slot 3, has no name"):
        r.input_many([(3, b";x\n")])
    r.update(1, login=1)
    with pytest.raises(ValueError, match=r"^read 2: .*slot 1, is still logging in"):
        r.input_many([GOOD, GOOD, (1, b".shout x\n")])
    r.update(0, room=None)
    with pytest.raises(ValueError, match=r"^read 0: .*no room"):
        r.input_many([GOOD])


def test_recording_needs_every_speaker_in_a_ring_room(no_library):
    r = seated(review_rooms=2)
    r.update(1, room=2)
    # the device decides which reads are says and emotes: even a read that can never be recorded is refused
    for data in (b"a say\n", b".shout never recorded\n", b"\xff\xfb\x01", b"\n"):
        with pytest.raises(ValueError, match=r"^read 1: .*room 2 has no review ring"):
            r.input_many([GOOD, (1, data)], record=True)
    with pytest.raises(ValueError, match=r"^read 0: .*no review ring.*review_rooms is 0"):
        seated().input_many([GOOD], record=True)
    assert r._prepare_input([GOOD, (0, b";waves\n")], True, True)[-2:] == (1, 1)
    assert r._prepare_input([GOOD, (1, b"anything\n")], False, False)[-2:] == (0, 0)


def test_a_closed_roster_raises(no_library):
    with seated() as r:
        pass
    with pytest.raises(ValueError, match="closed"):
        r.input_many([GOOD])
    with pytest.raises(ValueError, match="closed"):
        r.update(0, level=1)


# ---------------------------------------------- Roster.update(level=)
@pytest.mark.parametrize("fields", [
    {"level": -1}, {"level": 5}, {"level": None}, {"level": True}, {"level": 1.0}, {"level": "1"}, {"level": [1]},
    {"level": [1, 2, 3]}, {"level": [1, 9]}, {"level": 2, "vis": 7}, {"level": 2, "room": -4}, {"level": 9, "colour": 1},
    {"name": b"", "level": 3},
])
def test_a_rejected_update_changes_nothing(no_library, fields):
    r = seated()
    r.update([0, 1], level=[2, 3], muzzled=[0, 1])
    r._dirty = r._speech_dirty = False
    table, speech = r._table.copy(), r._speech.copy()
    with pytest.raises(ValueError):
        r.update([0, 1], **fields)
    assert np.array_equal(r._table, table) and np.array_equal(r._speech, speech)
    assert r._dirty is False and r._speech_dirty is False


def test_level_lands_in_byte_14_and_leaves_the_table_alone(no_library):
    r = device.Roster(5)
    assert not r._speech[:, 14].any()                                   # NEW at first
    r._dirty = r._speech_dirty = False
    r.update([1, 3, 1], level=[4, 2, 1])
    assert r._dirty is False and r._speech_dirty is True                # the speech mirror alone
    assert r._speech[:, 14].tolist() == [0, 1, 0, 2, 0]                 # the last value wins
    assert r._speech[:, 13].tolist() == [1] * 5 and not r._speech[:, :13].any() and not r._speech[:, 15].any()
    r.update(0, name=b"Al", level=np.int64(3), command_mode=1)
    assert r._speech[0].tobytes() == b"Al" + b"\0" * 10 + bytes([2, 5, 3, 0])
    r._speech_dirty = False
    r.update(2, room=3)
    assert r._dirty is True and r._speech_dirty is False
    r._dirty = False
    r.update(2, colour=1, level=0)                                      # both kinds of field: both mirrors
    assert r._dirty is True and r._speech_dirty is True
    r.update(range(5), level=4)
    assert r._speech[:, 14].tolist() == [4] * 5


# ---------------------------------------------- the kernel's command table
def test_the_kernels_command_table_is_the_restatements():
    source = device.SOURCE.read_text()
    table = source[source.index("kCommands[kNumCommands] = {"):]
    table = table[:table.index("};")]
    levels = {"kNew": 0, "kUser": 1, "kWiz": 2, "kArch": 3, "kGod": 4}
    got = [(name.encode(), levels[lv]) for name, lv in re.findall(r'cmd\("([a-z]+)", (k[A-Za-z]+)\)', table)]
    assert got == command_table() and len(got) == device.NUM_COMMANDS == 92
    assert max(len(name) for name, _ in got) == 10 == int(re.search(r"kNameMax = (\d+);", source).group(1))
    lib = nuts_path.lib()
    assert [lib.np_command_lookup(w) for w in (b"tell", b"pemote", b"echo", b"shout", b"emote", b"semote", b"say")] == \
        [5, 8, 9, device.COM_SHOUT, device.COM_EMOTE, device.COM_SEMOTE, device.COM_SAY]


# ---------------------------------------------- the model is the reference
@pytest.mark.parametrize("name", GOLDEN)
def test_the_dispatch_model_reproduces_what_every_client_received(name):
    res = replay_reads(name, model_answer)
    assert res["mismatches"] == []
    assert res["comparisons"] == GOLDEN_COMPARISONS[name]               # it cannot pass by skipping
    assert sum(GOLDEN_COMPARISONS.values()) == 86


def errors_session():
    """tests/golden/errors.json replayed through dispatch(): per line step the actor's speaker, the read, the model's
    verdict and what the actor received."""
    doc = json.loads((REPO / "tests" / "golden" / "errors.json").read_text())
    accounts = {acc["name"]: acc for group in doc["accounts"] for acc in (group if isinstance(group, list) else [group])}
    speakers, rows, other = {}, [], []
    for i, step in enumerate(doc["steps"]):
        if step["op"] == "login":
            acc = accounts[step["name"]]
            speakers[step["actor"]] = {"slot": len(speakers), "room": 0, "name": acc["name"].encode(), "vis": 1,
                                       "muzzled": int(bool(acc["muzzled"])), "command_mode": int(bool(acc["command_mode"])),
                                       "level": int(acc["level"])}
        elif step["op"] == "line" and step["actor"] in speakers:
            sp = speakers[step["actor"]]
            d, m = answer_of(sp, step["send"].encode("latin-1") + b"\n", False)
            rows.append((step["send"], sp, d, m, step["recv"].get(step["actor"], "")))
            if d["kind"] == COMMAND and nuts_path.lib().np_command_name(d["com"]) == b"mode":
                sp["command_mode"] ^= 1
        else:
            other.append((i, step))
    return doc, rows, other


def test_unknown_in_the_recorded_errors_is_exactly_what_the_model_calls_unknown():
    doc, rows, other = errors_session()
    wire = "Unknown command.\n\r"
    occurrences = json.dumps(doc).count("Unknown command.")
    assert occurrences == 5                                             # pinned from the file
    # an occurrence outside a plain line step of a logged-in user would be one the model never sees: name it
    strays = [(i, step.get("op"), step.get("send")) for i, step in other
              if "Unknown command." in json.dumps(step.get("recv", {}))]
    assert strays == []
    received = [send for send, sp, d, m, recv in rows if recv.startswith(wire)]
    called = [send for send, sp, d, m, recv in rows if d["kind"] == UNKNOWN]
    assert received == called and len(called) == occurrences            # both directions, and all five
    assert {".bogus command", ". "} < set(called)
    for send, sp, d, m, recv in rows:
        if d["kind"] == UNKNOWN:
            assert m["reply"] == UNKNOWN_NOTICE and m["line"] is None and m["outcome"] == device.NOT_SPEECH
            assert recv.count(wire) == 1
        else:
            assert wire not in recv, send
    # the level check and command mode are among them
    assert ".shout but not shout" in called and "hello" in called


def test_the_forced_say_and_the_empty_emotes_of_the_recorded_errors():
    _, rows, _ = errors_session()
    by_send = {send: (sp, d, m, recv) for send, sp, d, m, recv in rows}
    sp, d, m, recv = by_send[".say"]
    assert d["kind"] == SPEECH and d["com"] == SAY and d["forced"] and not sp["command_mode"]
    assert m["outcome"] == device.NOTHING and m["reply"] == WHAT_NOTICE[SAY] and recv == "Say what?\n\r"
    sp, d, m, recv = by_send["say"]                                     # the same through command mode
    assert d["forced"] and sp["command_mode"] and recv.startswith("Say what?\n\r")
    for send, com in ((";", EMOTE), ("#", SEMOTE)):
        sp, d, m, recv = by_send[send]
        assert d["kind"] == SPEECH and d["com"] == com and not d["forced"] and (d["start"], d["size"]) == (0, 1)
        assert m["outcome"] == device.NOTHING and m["reply"] == WHAT_NOTICE[com]      # the speech model's verdict
        assert recv == WHAT_NOTICE[com].decode().replace("\n", "\n\r")
    sp, d, m, recv = by_send[".shout"]
    assert d["kind"] == SPEECH and d["com"] == SHOUT and d["size"] == 0 and m["outcome"] == device.NOTHING
    # every speech step of the session, whatever its outcome, is what its actor received
    checked = 0
    for send, sp, d, m, recv in rows:
        if d["kind"] == SPEECH:
            want = b"".join(nuts_path.chunks(m["reply"], 0)) if m["reply"] is not None else b""
            assert recv.encode("latin-1").startswith(want) and (want or m["line"] is not None), send
            checked += 1
    assert checked == 12     # .shout .say ; # / Bobby's five muzzled ones less tell and echo / Carol's say / Dave's three


def test_the_dispatch_order_on_chosen_reads():
    user = {"command_mode": 0, "level": 1}
    com_mode = {"command_mode": 1, "level": 1}
    new = {"command_mode": 0, "level": 0}
    kind = lambda sp, data: dispatch(sp, data)["kind"]
    assert kind(user, b"\xff\xfb\x01") == IAC and kind(user, b"\n") == EMPTY and kind(user, b"   \r\n") == EMPTY
    assert kind(user, b".\n") == REPEAT and kind(user, b". \n") == UNKNOWN and kind(user, b" .\n") == SPEECH
    assert kind(com_mode, b" .\n") == UNKNOWN and kind(user, b"..\n") == UNKNOWN
    for data in (b"!x\n", b".!\n", b".;\n", b">x\n"):
        assert kind(user, data) == UNKNOWN, data
    assert kind(user, b" ;x\n") == SPEECH and dispatch(user, b" ;x\n")["com"] == SAY      # a say of " ;x"
    assert kind(com_mode, b" ;x\n") == UNKNOWN
    assert dispatch(user, b";x y\n") == {"kind": SPEECH, "com": EMOTE, "word_count": 2, "line_size": 4, "start": 0,
                                         "size": 4, "forced": False}
    assert dispatch(user, b"! loud  now\x80tail\n")["com"] == SHOUT and dispatch(user, b"! loud  now\x80tail\n")["start"] == 2
    assert [dispatch(user, s + b" bobby hi\n")["com"] for s in (b">", b"<", b"-")] == [5, 8, 9]
    assert dispatch(user, b".s hi\n")["com"] == SAY and dispatch(user, b".sh hi\n")["com"] == SHOUT
    assert dispatch(user, b".se hi\n")["com"] == SEMOTE and dispatch(com_mode, b"s\n")["forced"]
    assert kind(new, b";x\n") == UNKNOWN and kind(new, b".shout x\n") == UNKNOWN and kind(new, b"hi\n") == SPEECH
    assert kind(user, b".shutdown\n") == UNKNOWN and kind({"command_mode": 0, "level": 4}, b".shutdown\n") == COMMAND
    d = dispatch(user, b"." + b"w" * 40 + b" x\n")                      # a 39-byte comword matches nothing
    assert d["kind"] == UNKNOWN and d["word_count"] == 3
    assert dispatch(user, b" ".join([b"w"] * 9) + b"\n")["word_count"] == 9
    assert dispatch(user, b" ".join([b"w"] * 10) + b"\n")["word_count"] == 9
    assert dispatch(user, b"w" * 390 + b"\n")["word_count"] == 9 and dispatch(user, b"w" * 78 + b"\n")["word_count"] == 2
    # np_remove_first skips the whole first run, whatever its length
    d = dispatch(user, b".shout" + b"x" * 60 + b"  rest\n")
    assert d["kind"] == UNKNOWN
    d = dispatch(com_mode, b"sh" + b"\n")
    assert d["com"] == SHOUT and (d["start"], d["size"]) == (2, 0)


# ---------------------------------------------- the kernel's rules
def rule_reads(seed: int, n: int):
    rng = random.Random(seed)
    reads = systematic_reads() + [fuzz_read(rng) for _ in range(n)]
    modes = [rng.random() < 0.4 for _ in reads]
    levels = [rng.choice((0, 1, 1, 1, 2, 3, 4)) for _ in reads]
    return reads, modes, levels


def test_the_kernels_rules_equal_the_restatement():
    reads, modes, levels = rule_reads(1741, 100_000)
    assert len(reads) >= 100_000 and max(map(len, reads)) == 1000 and min(map(len, reads)) == 1
    fields = ("kind", "com", "word_count", "line_size", "start", "size", "forced")
    kinds = dict.fromkeys(KINDS, 0)
    seen = {"total_9": 0, "total_10_or_more": 0, "forced": 0, "high_terminator": 0, "high_inside": 0, "nul_inside": 0,
            "leading_blank": 0, "level_refused": 0}
    coms = set()
    for lo in range(0, len(reads), 4000):
        batch, mode, level = reads[lo:lo + 4000], modes[lo:lo + 4000], levels[lo:lo + 4000]
        got = parse_rule(batch, mode, level)
        for i, data in enumerate(batch):
            sp = {"command_mode": int(mode[i]), "level": level[i]}
            want = dispatch(sp, data)
            have = {f: (bool(got[f][i]) if f == "forced" else int(got[f][i])) for f in fields}
            assert have == want, (data, sp)
            kinds[want["kind"]] += 1
            coms.add(want["com"])
            n = want["line_size"]
            words = len(data[:n].split())
            seen["total_9"] += words == 9
            seen["total_10_or_more"] += words >= 10 and want["word_count"] == 9
            seen["forced"] += want["forced"]
            seen["high_terminator"] += data[n] >= 0x80 and data[0] != 255
            seen["high_inside"] += any(b >= 0x80 for b in data[n + 1:])
            seen["nul_inside"] += 0 in data[:-1]
            seen["leading_blank"] += data[:1] == b" " and want["word_count"] > 0
            seen["level_refused"] += (want["kind"] == UNKNOWN and n > 1 and
                                      dispatch({**sp, "level": 4}, data)["kind"] in (SPEECH, COMMAND))
    assert all(n >= 2000 for n in kinds.values()), kinds                # every kind, thousands of times
    assert all(n >= 100 for n in seen.values()), seen
    assert coms == set(range(-1, 92))                                   # every command was found, and none


def test_the_rule_inputs_cover_the_edges():
    edges = systematic_reads()
    table = command_table()
    have = set(edges)
    for name, _ in table:
        for cut in range(1, len(name) + 1):
            assert b".%s\n" % name[:cut] in have and b"%s\n" % name[:cut] in have
    terminators = {next(i for i, b in enumerate(r) if b < 32 or b >= 128) for r in edges}
    assert {0, 999} <= terminators
    assert all({16 * s - 1, 16 * s, 16 * s + 1} <= terminators for s in range(1, 62))
    runs = {len(w) for r in edges for w in r[:-1].split() if set(w) <= {ord("r")}}
    assert {38, 39, 40, 77, 78, 79, 390} <= runs
    for form in (b"!x\n", b".!\n", b" ;x\n", b"..\n", b". \n", b"\xff", b"ab\0cd\n"):
        assert form in have
    assert all(1 <= len(r) <= 1000 and not 32 <= r[-1] < 128 for r in edges)
    lib = nuts_path.lib()
    assert lib.np_command_count() == 92


# ---------------------------------------------- the dataclass
def hand_built_input():
    """An Input from the model alone for six reads, one of each kind, its Speech empty of everything but outcomes and
    one reply."""
    speaker = {"slot": 2, "room": 0, "name": b"Two", "vis": 1, "muzzled": 0, "command_mode": 0, "level": 1}
    datas = [b"\xff\xfd\x01", b"  \n", b".\n", b".bogus x\n", b".shout hello  there\r\n", b".look around\n", b"plain say\n"]
    k = len(datas)
    models = [answer_of(speaker, d, False) for d in datas]
    ds = [d for d, _ in models]
    texts = np.full(400, 0xAA, dtype=np.uint8)
    tstarts, tsizes = np.zeros((2, k), dtype=np.int64), np.full((2, k), -1, dtype=np.int64)
    at = 5
    for j, (_, m) in enumerate(models):
        for row, text in enumerate((m["line"], m["reply"])):
            if text is not None:
                tstarts[row, j], tsizes[row, j] = at, len(text)
                texts[at:at + len(text)] = np.frombuffer(text, dtype=np.uint8)
                at += len(text) + 3
    zeros = lambda *shape, dtype=np.int64: np.zeros(shape, dtype=dtype)
    plan = lambda: device.Plan(capacity=4, admitted_bits=zeros(k, 1, dtype=np.uint64), colour_bits=zeros(1, dtype=np.uint64),
                               variants=zeros(1, dtype=np.uint8), variant_starts=zeros(k, 2), variant_sizes=zeros(k, 2),
                               write_counts=zeros(k, 2, dtype=np.int32),
                               write_sizes=zeros(k, 2, device.MAX_WRITES, dtype=np.int32))
    speech = device.Speech(outcome=np.array([m["outcome"] for _, m in models], dtype=np.int8), room=plan(), reply=plan(),
                           texts=texts, text_starts=tstarts, text_sizes=tsizes)
    inp = device.Input(kind=np.array([d["kind"] for d in ds], dtype=np.int8), com=np.array([d["com"] for d in ds], dtype=np.int8),
                       word_count=np.array([d["word_count"] for d in ds], dtype=np.uint8),
                       line_sizes=np.array([d["line_size"] for d in ds], dtype=np.int32),
                       inpstr_starts=np.array([d["start"] for d in ds], dtype=np.int64),
                       inpstr_sizes=np.array([d["size"] for d in ds], dtype=np.int64), speech=speech, data=datas)
    return inp, datas, models


def test_a_hand_built_input_obeys_its_accessors(no_library):
    inp, datas, models = hand_built_input()
    assert inp.kind.tolist() == [IAC, EMPTY, REPEAT, UNKNOWN, SPEECH, COMMAND, SPEECH] and inp.timing == {}
    assert inp.com.tolist() == [-1, -1, -1, -1, SHOUT, 1, SAY] and inp.word_count.tolist() == [0, 0, 1, 2, 3, 2, 2]
    assert inp.inpstr_sizes.tolist() == [-1, -1, -1, -1, 12, 6, 9]
    assert [inp.inpstr(k) for k in range(7)] == [b"", b"", b"", b"", b"hello  there", b"around", b"plain say"]
    assert [inp.line(k) for k in range(7)] == [b"", b"  ", b".", b".bogus x", b".shout hello  there", b".look around",
                                               b"plain say"]
    assert inp.speech.outcome.tolist() == [-1, -1, -1, -1, device.SPOKEN, -1, device.SPOKEN]
    assert inp.speech.reply_text(3) == UNKNOWN_NOTICE and inp.speech.line(3) == b""
    assert inp.speech.line(4) == b"~OLTwo shouts:~RS hello  there\n" and inp.speech.line(6) == b"Two says: plain say\n"
    assert all(inp.speech.line(k) == b"" and inp.speech.reply_text(k) == b"" for k in (0, 1, 2, 5))
    for bad_k in (-1, 7):
        with pytest.raises(IndexError):
            inp.inpstr(bad_k)
        with pytest.raises(IndexError):
            inp.line(bad_k)
        with pytest.raises(IndexError):
            inp.speech.line(bad_k)


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def input_run(built):
    res = child_run.run_child("device_input_child.py", "DEVICE_INPUT", 600)
    print("\n[input]", json.dumps(res)[:4000])
    return res


@pytest.mark.gpu
def test_the_golden_sessions_replay_through_input_many(input_run):
    g = input_run["golden"]
    assert list(g) == list(GOLDEN)
    for name in GOLDEN:
        assert g[name]["comparisons"] == GOLDEN_COMPARISONS[name], name
        assert g[name]["mismatches"] == [] and g[name]["n_bad_vs_model"] == 0, (name, g[name])
    assert sum(g[name]["comparisons"] for name in GOLDEN) == 86


@pytest.mark.gpu
def test_seeded_reads_match_the_model(input_run):
    f = input_run["fuzz"]
    assert f["capacities"] == list(CAPACITIES) == [1, 63, 64, 65, 300, 1000]
    assert f["calls"] == 2 * len(CAPACITIES) and f["reads"] == f["calls"] * READS_PER_CALL and READS_PER_CALL >= 200
    assert f["longest_read"] == 1000
    assert all(f["kinds"].get(str(kind), 0) > 0 for kind in KINDS), f["kinds"]
    by = f["outcome_by_com"]
    for outcome in (device.SPOKEN, device.MUZZLED, device.NOTHING, device.SWEARING):
        for com in COMS:
            if (outcome, com) == (device.SWEARING, SEMOTE):
                assert f"{outcome}/{com}" not in by                     # semote has no swear check
            else:
                assert by.get(f"{outcome}/{com}", 0) > 0, (outcome, com, by)
    assert f["forced"] > 0
    assert f["n_bad"] == 0, f["first_bad"]


@pytest.mark.gpu
def test_a_speech_read_is_speak_many_of_its_parsed_event(input_run):
    c = input_run["contract"]
    assert c["checked"] >= 100 and c["coms"] == sorted(COMS) and c["forced_skipped"] > 0
    assert c["n_bad"] == 0, c["first_bad"]


@pytest.mark.gpu
def test_recording_through_input_many_is_recording_the_parsed_events(input_run):
    r = input_run["recording"]
    assert r["input_calls"] >= 15 and r["speak_calls"] >= 10 and r["clears"] >= 3 and r["reviews"] >= 5
    assert r["recorded"] > 100 and r["lines_compared"] > 100 and r["most_into_one_room_in_one_call"] > 15
    assert r["n_bad"] == 0, r["first_bad"]


@pytest.mark.gpu
def test_nothing_else_moved(input_run):
    m = input_run["moved"]
    cap = m["capacity"]
    for later in ("after_input", "after_level_update_again", "after_input_again"):
        assert m[later] == m["before"], later                           # results and copy volumes alike
    # right after the level update speak_many, and it alone, carries the speaker table once; every result is the same
    upd, before = m["after_level_update"], m["before"]
    assert {f: upd[f] for f in upd if f != "copies"} == {f: before[f] for f in before if f != "copies"}
    assert [upd["copies"][i] for i in (0, 1, 3)] == [before["copies"][i] for i in (0, 1, 3)]
    assert 16 * cap <= upd["copies"][2][0] - before["copies"][2][0] < 16 * cap + 256 and upd["copies"][2][1] == before["copies"][2][1]
    assert m["level_update_left_dirty"] == [False, False]
    h = m["input_h2d"]
    assert len(set(h["clean"])) == 1 and len(m["input_d2h"]) == 1       # the copies depend on the reads alone
    assert 16 * cap <= h["after_level_update"] - h["clean"][0] < 16 * cap + 256           # the speaker table alone
    # the table alone, in its two 256-byte aligned slices: the speaker table behind it was not given and does not travel
    assert 5 * cap <= h["after_table_update"] - h["clean"][0] < 5 * cap + 512 < 16 * cap
