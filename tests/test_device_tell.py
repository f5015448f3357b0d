"""``Roster.tell_many``: tell() and pemote() with get_user() on the device (nuts_roster_tell of fanout.hip),
``device.Private``, the ``afk`` / ``igntell`` / ``afk_mesg`` fields of ``Roster.update``, and the revtell rings
(``Roster(revtell=True)``, ``revtell_many``, ``clear_revtell``; nuts_roster_record_tell, nuts_roster_revtell).

Host tier (unmarked): everything malformed is rejected before the device library loads, and a rejected update changes
no mirror; the speaker record's layout byte for byte; the Python model of the command functions (``private`` of
tests/device_tell_child.py) reproduces what every client received at every step of nine recorded sessions that
dispatches to tell or pemote, and at both ``.revtell`` steps; a composed private text fits its slot, ``TEXT_SIZE`` and the
variant bounds, a stored line the line bounds; the kernel's lookup, stated in numpy with a row per slot and two minima,
equals the sequential ``get_user`` on more than 100,000 seeded (roster, word) pairs; a ``Private`` built by hand obeys
its contract.  The kernels' scratch-free compile is tests/test_device_fanout.py's, over every name in ``device.KERNELS``.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_tell_child.py, under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import json
import random
from pathlib import Path

import numpy as np
import pytest

import child_run
from device_tell_child import (AFK, CAPACITIES, COMS, EVENTS_PER_CALL, GOLDEN, GOLDEN_COMPARISONS, GOLDEN_PRIVATE_STEPS,
                               IGNALL, IGNTELL, MUZZLED, MUZZLED_NOTICE, NOBODY, NOBODY_NOTICE, NOTHING, OFFSITE, OUTCOMES,
                               PEMOTE, SELF, SELF_NOTICE, TELL, TOLD, WHAT_NOTICE, TellRings, get_user, lookup_rule,
                               model_answers, new_user, packed_names, private, replay_private, word_1)
from nuts333_amd import device, nuts_path

REPO = Path(__file__).resolve().parent.parent


def seated(capacity=4, **kw) -> device.Roster:
    """A roster whose slots 0 and 1 can speak: a room and a name."""
    r = device.Roster(capacity, **kw)
    r.update([0, 1], room=0, name=[b"Alice", "Bobby"])
    return r


GOOD = (0, TELL, b"bobby hello there", 4)


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


# ------------------------------------------------------------------ host tier: input checks
def test_the_new_names_exist():
    assert {"nuts_roster_tell", "nuts_roster_record_tell", "nuts_roster_revtell"} <= set(device.KERNELS)
    assert device.KERNELS[:14] == ("nuts_fanout_measure_broadcast", "nuts_fanout_emit_broadcast", "nuts_fanout_measure_batch",
                                   "nuts_fanout_emit_batch", "nuts_fanout_measure_many", "nuts_fanout_emit_many",
                                   "nuts_roster_measure", "nuts_roster_emit", "nuts_roster_plan", "nuts_roster_record",
                                   "nuts_roster_review", "nuts_roster_speak", "nuts_roster_speak_plan", "nuts_roster_parse")
    assert (device.COM_TELL, device.COM_PEMOTE) == (5, 8)
    assert (device.SPOKEN, device.MUZZLED, device.NOTHING, device.SWEARING) == (0, 1, 2, 3)
    assert OUTCOMES == (0, 1, 2, 4, 5, 6, 7, 8, 9)
    assert device.SPEECH_FLAGS == {"vis": 1, "muzzled": 2, "command_mode": 4, "afk": 8, "igntell": 16}
    assert device.AFK_MESG_LEN == 60 and device.REVTELL_LINES == 5
    assert (device.MAX_REVTELL_BYTES, device.MAX_REVTELL_WRITES) == (5 * 1210, 15)


@pytest.mark.parametrize("events", [[], (), None, 3, "tell", b"tell", np.zeros(3)])
def test_events_must_be_a_non_empty_sequence(no_library, events):
    with pytest.raises(ValueError, match="events|empty call"):
        seated().tell_many(events)


@pytest.mark.parametrize("bad, why", [
    ([0, TELL, b"x", 3], "tuple"), ((0, TELL, b"x"), "tuple"), ((0, TELL, b"x", 3, 0), "tuple"),
    ((4, TELL, b"x", 3), "slot"), ((-1, TELL, b"x", 3), "slot"), ((None, TELL, b"x", 3), "slot"), ((True, TELL, b"x", 3), "slot"),
    ((0, 3, b"x", 3), "com"), ((0, 4, b"x", 3), "com"), ((0, 0, b"x", 3), "com"), ((0, "tell", b"x", 3), "com"),
    ((0, True, b"x", 3), "com"), ((0, 5.0, b"x", 3), "com"), ((0, 92, b"x", 3), "com"),
    ((0, TELL, b"a\0b", 3), "NUL"), ((0, TELL, 5, 3), "text must be"), ((0, PEMOTE, "Ā", 3), "outside one byte"),
    ((0, TELL, b"x" * 1000, 3), "at most 999"), ((0, PEMOTE, "y" * 1999, 3), "at most 999"),
    ((0, TELL, b"x", -1), "word_count"), ((0, TELL, b"x", 11), "word_count"), ((0, TELL, b"x", 1.0), "word_count"),
    ((0, TELL, b"x", None), "word_count"), ((0, TELL, b"x", True), "word_count"),
])
def test_a_malformed_event_is_rejected_by_its_number(no_library, bad, why):
    with pytest.raises(ValueError, match=rf"^event 1: .*{why}"):
        seated().tell_many([GOOD, bad, GOOD])


def test_the_longest_inpstr_and_every_word_count_pass_the_checks(no_library):
    r = seated()
    for com in COMS:
        packed = r._prepare_private([(1, com, b"x" * 999, wc) for wc in range(11)] + [(0, com, "", 0)], False)
        assert packed[2].tolist() == [999] * 11 + [0] and packed[5].tolist() == list(range(11)) + [0]
        assert packed[3].tolist() == [1] * 11 + [0] and set(packed[4].tolist()) == {com} and packed[6] == 0


@pytest.mark.parametrize("bad", [2, -1, None, "yes", 1.0, [True]])
def test_record_must_be_a_bool(no_library, bad):
    with pytest.raises(ValueError, match="record"):
        seated(revtell=True).tell_many([GOOD], record=bad)


def test_there_is_no_ban_swearing_argument(no_library):
    with pytest.raises(TypeError):
        seated().tell_many([GOOD], ban_swearing=True)


def test_recording_needs_revtell_rings(no_library):
    with pytest.raises(ValueError, match="revtell"):
        seated().tell_many([GOOD], record=True)
    assert seated(revtell=True)._prepare_private([GOOD], True)[6] == 1
    for call in (lambda r: r.revtell_many([0]), lambda r: r.clear_revtell(0), lambda r: r.clear_revtell([0, 1])):
        with pytest.raises(ValueError, match="revtell"):
            call(seated())
    for bad in (2, "yes", None, 1):
        with pytest.raises(ValueError, match="revtell"):
            device.Roster(4, revtell=bad)


def test_the_speaker_needs_a_room_a_name_and_no_login(no_library):
    r = seated()
    r.update(2, name=b"Carol")                           # no room: it can be told (OFFSITE), but cannot tell
    r.update(3, room=0)                                  # no name
    with pytest.raises(ValueError, match=r"^event 1: .*slot 2, has no room"):
        r.tell_many([GOOD, (2, TELL, b"alice x", 3)])
    with pytest.raises(ValueError, match=r"^event 0: .*slot 3, has no name"):
        r.tell_many([(3, PEMOTE, b"alice x", 3)])
    r.update(1, login=1)
    with pytest.raises(ValueError, match=r"^event 2: .*slot 1, is still logging in"):
        r.tell_many([GOOD, GOOD, (1, TELL, b"alice x", 3)])


def test_the_revtell_calls_check_their_slots(no_library):
    r = seated(revtell=True)
    for bad in ([], (), "0", None, 3):
        with pytest.raises(ValueError, match="slots|empty call"):
            r.revtell_many(bad)
    for bad in ([4], [-1], [0, None], [True], [1.0]):
        with pytest.raises(ValueError, match="slot"):
            r.revtell_many(bad)
        with pytest.raises(ValueError, match="slot"):
            r.clear_revtell(bad)
    assert not r._tell_clear_pending and not r._tell_clear.any()
    r.clear_revtell([])
    assert not r._tell_clear_pending
    r.clear_revtell([1, 3, 1])
    r.clear_revtell(0)
    assert r._tell_clear.tolist() == [1, 1, 0, 1] and r._tell_clear_pending
    assert not r._clear_pending                                         # the rooms' rings are another matter


def test_a_closed_roster_raises(no_library):
    with seated(revtell=True) as r:
        pass
    for call in (lambda: r.tell_many([GOOD]), lambda: r.revtell_many([0]), lambda: r.clear_revtell(0),
                 lambda: r.update(0, afk=1)):
        with pytest.raises(ValueError, match="closed"):
            call()


@pytest.mark.parametrize("fields", [
    {"afk": 2}, {"afk": "1"}, {"afk": None}, {"afk": [1]}, {"afk": [0, 1, 0]}, {"igntell": -1}, {"igntell": [0, 2]},
    {"igntell": 1.0}, {"afk_mesg": b"x" * 61}, {"afk_mesg": b"a\0b"}, {"afk_mesg": 5}, {"afk_mesg": None},
    {"afk_mesg": "Ā"}, {"afk_mesg": [b"ok"]}, {"afk_mesg": [b"ok", b"fine", b"three"]}, {"afk_mesg": [b"ok", b"y" * 61]},
    {"afk": 1, "igntell": 1, "afk_mesg": b"fine", "muzzled": 7}, {"afk_mesg": b"fine", "room": -4},
    {"afk": 1, "name": b""}, {"igntell": 1, "colour": 3}, {"afk_mesg": b"fine", "level": 5},
])
def test_a_rejected_update_changes_no_mirror(no_library, fields):
    r = seated()
    r.update([0, 1], afk=[1, 0], igntell=[0, 1], afk_mesg=[b"back soon", b""])
    r._dirty = r._speech_dirty = r._private_dirty = r._afk_dirty = False
    table, speech, afk = r._table.copy(), r._speech.copy(), r._afk.copy()
    with pytest.raises(ValueError):
        r.update([0, 1], **fields)
    assert np.array_equal(r._table, table) and np.array_equal(r._speech, speech) and np.array_equal(r._afk, afk)
    assert (r._dirty, r._speech_dirty, r._private_dirty, r._afk_dirty) == (False, False, False, False)


def test_the_speaker_record_byte_for_byte_and_the_dirty_flags(no_library):
    r = device.Roster(5)
    assert r._speech.shape == (5, 16) and r._afk.shape == (5, 64) and r._afk.dtype == np.uint8 and not r._afk.any()
    assert r._speech[:, 13].tolist() == [1] * 5 and not r._speech[:, :13].any() and not r._speech[:, 14:].any()
    assert r._afk_dirty and r._speech_dirty and not r._private_dirty
    r._dirty = r._speech_dirty = r._afk_dirty = False
    r.update([1, 3, 1], afk=[1, 1, 0], igntell=[0, 1, 1], afk_mesg=[b"first", "m" * 60, b"last"])
    # the table's and the speech calls' flags stay as they were: only tell_many uploads for these fields
    assert (r._dirty, r._speech_dirty, r._private_dirty, r._afk_dirty) == (False, False, True, True)
    assert r._speech[1].tobytes() == b"\0" * 13 + bytes([1 | 16, 0, 0])              # the last values win
    assert r._speech[3].tobytes() == b"\0" * 13 + bytes([1 | 8 | 16, 0, 0])
    assert r._afk[1].tobytes() == b"last" + b"\0" * 56 + bytes([4, 0, 0, 0])
    assert r._afk[3].tobytes() == b"m" * 60 + bytes([60, 0, 0, 0]) and not r._afk[[0, 2, 4]].any()
    r.update(1, afk_mesg=b"")
    assert not r._afk[1].any()
    r._private_dirty = r._afk_dirty = False
    r.update(3, name=b"Abcdefghijkl", vis=0, muzzled=1, command_mode=1, level=4, afk=0)
    assert r._speech[3].tobytes() == b"Abcdefghijkl" + bytes([12, 2 | 4 | 16, 4, 0])  # bytes 0..12, 14, 15 as they were
    assert (r._dirty, r._speech_dirty, r._private_dirty, r._afk_dirty) == (False, True, True, False)
    r._speech_dirty = r._private_dirty = False
    r.update(2, afk_mesg=b"x")
    assert (r._dirty, r._speech_dirty, r._private_dirty, r._afk_dirty) == (False, False, False, True)
    r.update(2, room=3, igntell=1)                                      # both kinds of field: both mirrors
    assert (r._dirty, r._speech_dirty, r._private_dirty) == (True, False, True)
    assert r._table.nbytes == 5 * 5                                     # the 5-byte-per-slot table is what it was


# ---------------------------------------------- the model is the reference
@pytest.mark.parametrize("name", GOLDEN)
def test_the_model_reproduces_what_every_client_received(name):
    res = replay_private(name, *model_answers())
    assert res["mismatches"] == []
    assert res["private_steps"] == GOLDEN_PRIVATE_STEPS[name]           # it cannot pass by skipping
    assert res["comparisons"] == GOLDEN_COMPARISONS[name]
    assert sum(GOLDEN_PRIVATE_STEPS.values()) == 38 >= 37 and GOLDEN_PRIVATE_STEPS["review"] == 8 + 2


def test_the_replay_leaves_no_private_step_out():
    """Every line step whose first word is a tell or pemote form is one the replay answers, but for the one sent by a user
    whose level does not reach the command (exec_com answers ``Unknown command.``)."""
    for name in GOLDEN:
        steps = json.loads((REPO / "tests" / "golden" / f"{name}.json").read_text())["steps"]
        firsts = [s["send"].split()[0] for s in steps if s["op"] == "line" and s["send"].split()]
        forms = sum(f in (">", "<", ".revtell") or (len(f) > 1 and (".tell".startswith(f) and len(f) > 2 or ".pemote".startswith(f)))
                    for f in firsts)
        unknown = sum(s["op"] == "line" and s["send"].startswith(".tell") and list(s["recv"].values()) == ["Unknown command.\n\r"]
                      for s in steps)
        assert forms - unknown == GOLDEN_PRIVATE_STEPS[name], name


def test_the_outcomes_of_the_recorded_sessions_cover_every_notice():
    seen = {}
    for name in GOLDEN:
        for outcome, n in replay_private(name, *model_answers())["outcomes"].items():
            seen[int(outcome)] = seen.get(int(outcome), 0) + n
    assert set(seen) == {TOLD, MUZZLED, NOTHING, NOBODY, SELF, AFK, IGNALL, IGNTELL}     # OFFSITE needs a netlink
    assert seen[TOLD] >= 20


def people():
    users = {0: new_user(0, name=b"Alice"), 1: new_user(1, name=b"Bobby", level=3), 2: new_user(2, name=b"Alicia"),
             3: new_user(3, name=b"Bob"), 4: new_user(4, name=None), 5: new_user(5, name=b"Carol", room=None),
             6: new_user(6, name=b"Zed", login=1), 7: new_user(7, name=b"Zed")}
    return users


def test_the_order_of_the_checks_and_the_lookup():
    u = people()
    assert private(u, 0, TELL, b"bob hi", 3)["target"] == 3             # the exact match at 3 beats the substring at 1
    assert private(u, 0, TELL, b"bobb hi", 3)["target"] == 1
    assert private(u, 1, TELL, b"alic hi", 3)["target"] == 0             # two substring matches: the lowest
    assert private(u, 1, TELL, b"alici hi", 3)["target"] == 2
    assert private(u, 1, TELL, b"lic hi", 3)["outcome"] == NOBODY       # "Lic": the capital is written into the word
    assert private(u, 0, TELL, b"zed hi", 3)["target"] == 7             # the slot that is logging in is skipped
    assert private(u, 0, TELL, b"alic hi", 3)["outcome"] == SELF        # found oneself, by substring too
    assert private(u, 0, TELL, b"bOB hi", 3)["outcome"] == NOBODY       # only the first byte is capitalised
    assert private(u, 0, TELL, b"9 hi", 3)["outcome"] == NOBODY
    m = private(u, 0, TELL, b"carol hi", 3)
    assert (m["outcome"], m["target"], m["reply"]) == (OFFSITE, 5, b"Carol is offsite and would not be able to reply to you.\n")
    assert private(u, 0, PEMOTE, b"alice waves", 3) == {"outcome": SELF, "target": None, "reply": SELF_NOTICE[PEMOTE], "line": None}
    m = private(u, 0, PEMOTE, b"alic waves", 3)                         # through a substring a pemote reaches oneself
    assert (m["outcome"], m["target"], m["line"]) == (TOLD, 0, b"~OL>>~RS Alice waves\n")
    assert m["reply"] == b"~OL(To Alice)~RS Alice waves\n"
    assert private(u, 0, TELL, b"", 3)["outcome"] == SELF               # strstr finds the empty word in the first name
    assert private(u, 1, TELL, b"", 3)["target"] == 0
    assert private(u, 0, TELL, b"w" * 50 + b" x", 3)["outcome"] == NOBODY and word_1(b"w" * 50 + b" x") == b"w" * 39
    assert private(u, 0, TELL, b" \xe9 bobby  hello? ", 4)["reply"] == b"~OLYou tell Bobby:~RS hello? \n"
    assert private(u, 0, TELL, b"bobby is it?", 4)["line"] == b"~OLAlice asks you:~RS is it?\n"
    u[0]["vis"] = 0
    assert private(u, 0, TELL, b"bobby x", 3)["line"] == b"~OLA presence tells you:~RS x\n"
    u[0]["muzzled"] = 1
    assert private(u, 0, TELL, b"bobby x", 2)["reply"] == MUZZLED_NOTICE[TELL]       # muzzled before everything
    u[0]["muzzled"] = 0
    assert private(u, 0, PEMOTE, b"alice x", 2)["reply"] == WHAT_NOTICE[PEMOTE]      # then the word count
    # private_blocked in its order, on both sides of the level rule
    u[1].update(afk=1, ignall=1, igntell=1, room=None, afk_mesg=b"")
    assert private(u, 0, TELL, b"bobby x", 3)["reply"] == b"Bobby is AFK at the moment.\n"
    u[1]["afk_mesg"] = b"m" * 60
    assert private(u, 0, PEMOTE, b"bobby x", 3)["reply"] == b"Bobby is AFK, message is: " + b"m" * 60 + b"\n"
    u[1]["afk"] = 0
    for level, outcome in ((0, IGNALL), (1, IGNALL), (2, IGNALL), (3, OFFSITE), (4, OFFSITE)):    # Bobby is level 3
        u[0]["level"] = level
        assert private(u, 0, TELL, b"bobby x", 3)["outcome"] == outcome, level
    u[1]["ignall"] = 0
    for level, outcome in ((1, IGNTELL), (2, IGNTELL), (3, OFFSITE)):
        u[0]["level"] = level
        assert private(u, 0, PEMOTE, b"bobby x", 3)["outcome"] == outcome, level
    u[0]["level"] = 1
    assert private(u, 0, TELL, b"bobby x", 3)["reply"] == b"Bobby is ignoring tells at the moment.\n"
    assert private(u, 0, PEMOTE, b"bobby x", 3)["reply"] == b"Bobby is ignoring private emotes at the moment.\n"
    assert private(u, 0, TELL, b"nobody x", 3)["reply"] == NOBODY_NOTICE


# ---------------------------------------------- bounds
def fuzz_private(seed: int, n: int):
    """Seeded (users, slot, com, inpstr, wc) over small rosters of 12-byte and 1-byte names, visible and not."""
    rng = random.Random(seed)
    for _ in range(n):
        users = {j: new_user(j, name=rng.choice((b"Abcdefghijkl", b"A", b"Bobby", b"Qrstuvwxyzab")), vis=rng.randrange(2),
                             afk=int(rng.random() < 0.2), afk_mesg=rng.choice((b"", b"m" * 60, b"\n" * 60)),
                             ignall=int(rng.random() < 0.2), igntell=int(rng.random() < 0.2),
                             room=rng.choice((0, 0, None))) for j in range(4)}
        users[0]["room"] = 0
        word = rng.choice((b"", b"a", b"A", b"bobby", b"abcdefghijkl", b"qrstuvwxyzab", b"l", b"nobody", b"w" * 50))
        sep = rng.choice((b"", b" ", b"  ", b"\xe9"))
        rest = rng.choice((b"", b"x", b"?", b"\n" * 999, b"~FR" * 333, b"y" * 999, b"hello there?"))
        yield users, 0, rng.choice(COMS), (rng.choice((b"", b" ")) + word + sep + rest)[:999], rng.choice((3, 3, 3, 2))


def test_a_composed_private_text_fits_its_slot():
    most, longest_notice = 0, 0
    for users, slot, com, inpstr, wc in fuzz_private(7, 4000):
        m = private(users, slot, com, inpstr, wc)
        for text in (m["line"], m["reply"]):
            if text is None:
                continue
            assert len(text) <= len(inpstr) + device._TELL_SLACK == len(inpstr) + 96 and len(text) < device.TEXT_SIZE
            if m["outcome"] == TOLD:
                assert len(text) <= len(inpstr) + device.PRIVATE_EXTRA
                most = max(most, len(text) - len(inpstr))
            else:
                longest_notice = max(longest_notice, len(text))
    # the derivation: a pemote reply, 12-byte names on both sides, over an inpstr that holds nothing but the word -- an
    # empty one at the extreme, which strstr finds in the first name: the speaker's own here
    users = {0: new_user(0, name=b"Abcdefghijkl"), 1: new_user(1, name=b"Qrstuvwxyzab")}
    m = private(users, 0, PEMOTE, b"", 3)
    assert m["reply"] == b"~OL(To Abcdefghijkl)~RS Abcdefghijkl \n" and m["line"] == b"~OL>>~RS Abcdefghijkl \n"
    assert most <= len(m["reply"]) == 38 == device.PRIVATE_EXTRA and most >= 37
    assert len(private(users, 0, PEMOTE, b"q", 3)["reply"]) == 1 + 37                  # the figure of the issue
    # ... and the AFK notice, which holds nothing of inpstr: it has to fit beside an empty one
    assert longest_notice == len(b"Abcdefghijkl is AFK, message is: " + b"m" * 60 + b"\n") == 94 <= device._TELL_SLACK


def test_the_worst_private_texts_stay_within_the_variant_bounds():
    users = {0: new_user(0, name=b"Abcdefghijkl"), 1: new_user(1, name=b"Qrstuvwxyzab", afk_mesg=b"\n" * 60)}
    texts = []
    for rest in (b"\n" * 997, b"~FR" * 332, b"\n" * 996 + b"?", b"/~" * 498):
        for com in COMS:
            m = private(users, 0, com, b"q " + rest, 3)
            assert m["outcome"] == TOLD
            texts += [m["line"], m["reply"]]
    users[1]["afk"] = 1
    texts.append(private(users, 0, TELL, b"q x", 3)["reply"])
    ring = TellRings(1)
    for text in texts:
        assert len(text) < device.TEXT_SIZE
        for c in (0, 1):
            ch = nuts_path.chunks(text, c)
            assert sum(map(len, ch)) <= device.max_bytes(len(text)) and len(ch) <= device.MAX_WRITES
        ring.clear(0)
        ring.record(0, text)
        (stored,) = ring.lines(0)
        assert len(stored) <= device.REVIEW_LEN + 1
        for c in (0, 1):
            ch = nuts_path.chunks(stored, c)
            assert sum(map(len, ch)) <= device.MAX_LINE_BYTES and len(ch) <= device.MAX_LINE_WRITES
    assert device.REVTELL_LINES * device.MAX_LINE_BYTES == device.MAX_REVTELL_BYTES


# ---------------------------------------------- the kernel's lookup
def test_the_kernels_lookup_equals_the_sequential_get_user():
    rng = random.Random(1741)
    syll = (b"al", b"ice", b"bob", b"by", b"x", b"Zed", b"9", b"\xe9", b"an", b"na", b"A", b"B")
    pairs = found = exact_over_sub = 0
    for _ in range(260):
        cap = rng.choice((1, 2, 5, 17, 40))
        users = {}
        for j in range(cap):
            name = b"".join(rng.choice(syll) for _ in range(rng.randrange(1, 6)))[:12] if rng.random() < 0.9 else None
            if name and rng.random() < 0.7:
                name = name[:1].upper() + name[1:]
            users[j] = new_user(j, name=name, login=int(rng.random() < 0.15))
        names = [u["name"] for u in users.values() if u["name"]] or [b"Nobody"]
        words = []
        for _ in range(400):
            nm = rng.choice(names)
            x = rng.random()
            if x < 0.3:
                w = nm
            elif x < 0.7:
                a = rng.randrange(len(nm))
                w = nm[a:rng.randrange(a, len(nm) + 1)]
            elif x < 0.85:
                w = b"".join(rng.choice(syll) for _ in range(rng.randrange(0, 4)))
            else:
                w = rng.choice((nm + b"x", b"x" + nm, b"w" * 13, b"w" * 39, nm[:11] + b"\x7f", b""))
            w = bytes(b for b in w if 33 <= b < 128)[:39]              # a word holds only such bytes
            words.append(w[:1].lower() + w[1:] if rng.random() < 0.5 else w)
        got = lookup_rule(*packed_names(users, cap), words)
        for w, g in zip(words, got.tolist()):
            want = get_user(users, w)
            assert g == (-1 if want is None else want), (w, users)
            pairs += 1
            found += want is not None
            if want is not None and users[want]["name"] == (w[:1].upper() + w[1:]):
                exact_over_sub += any(u["name"] and not u["login"] and (w[:1].upper() + w[1:]) in u["name"]
                                      for j, u in users.items() if j < want)
    assert pairs >= 100_000 and found > 30_000 and pairs - found > 10_000 and exact_over_sub > 100


# ---------------------------------------------- the dataclass
def hand_built_private():
    """A Private from the model alone, for a 70-slot roster: texts and variants scattered over buffers of 0xAA bytes, -7
    in the unused chunk sizes."""
    cap, words = 70, 2
    users = {5: new_user(5, name=b"Five"), 66: new_user(66, name=b"Sixtysix", vis=0), 9: new_user(9, name=b"Nine", muzzled=1),
             30: new_user(30, name=b"Thirty", afk=1, afk_mesg=b"~FRaway"), 31: new_user(31, name=b"Fiver")}
    events = [(5, TELL, b"sixtysix ~FRred~RS hello?", 4), (66, PEMOTE, b"five waves", 3), (9, TELL, b"five mmph", 3),
              (5, TELL, b"thirty there?", 3), (5, TELL, b"five me", 3), (5, PEMOTE, b"fiv me", 3), (66, TELL, b"x", 2),
              (66, TELL, b"nobody at all", 4)]
    colour = np.arange(cap) % 3 == 0
    k = len(events)
    texts = np.full(4000, 0xAA, dtype=np.uint8)
    variants = np.full(40_000, 0xAA, dtype=np.uint8)
    tstarts, tsizes = np.zeros((2, k), dtype=np.int64), np.full((2, k), -1, dtype=np.int64)
    starts, sizes = np.zeros((2, k, 2), dtype=np.int64), np.zeros((2, k, 2), dtype=np.int64)
    counts = np.zeros((2, k, 2), dtype=np.int32)
    wsz = np.full((2, k, 2, device.MAX_WRITES), -7, dtype=np.int32)
    bits = np.zeros((2, k, words), dtype=np.uint64)
    outcome, target = np.zeros(k, dtype=np.int8), np.full(k, -1, dtype=np.int32)
    models, at, vat = [], 3, 7
    for j, (slot, com, inpstr, wc) in enumerate(events):
        m = private(users, slot, com, inpstr, wc)
        models.append(m)
        outcome[j] = m["outcome"]
        target[j] = -1 if m["target"] is None else m["target"]
        for row, (text, who) in enumerate(((m["line"], m["target"]), (m["reply"], slot))):
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
            bits[row, j, who // 64] = np.uint64(1) << np.uint64(who % 64)
    plans = [device.Plan(capacity=cap, admitted_bits=bits[i], colour_bits=device._pack(colour), variants=variants,
                         variant_starts=starts[i], variant_sizes=sizes[i], write_counts=counts[i], write_sizes=wsz[i])
             for i in (0, 1)]
    pv = device.Private(outcome=outcome, target=target, told=plans[0], reply=plans[1], texts=texts, text_starts=tstarts,
                        text_sizes=tsizes)
    return pv, events, models, colour


def test_a_hand_built_private_obeys_the_contract(no_library):
    pv, events, models, colour = hand_built_private()
    assert pv.outcome.tolist() == [TOLD, TOLD, MUZZLED, AFK, SELF, TOLD, NOTHING, NOBODY] and pv.timing == {}
    assert pv.target.tolist() == [66, 5, -1, 30, 5, 5, -1, -1]
    for k, ((slot, com, inpstr, wc), m) in enumerate(zip(events, models)):
        assert pv.line(k) == (m["line"] or b"") and pv.reply_text(k) == m["reply"] != b""
        for plan, text in ((pv.told, m["line"]), (pv.reply, m["reply"])):
            for c in (0, 1):
                assert plan.chunks(k, c) == (nuts_path.chunks(text, c) if text is not None else [])
                assert plan.variant(k, c) == b"".join(plan.chunks(k, c))
        assert pv.reply.admitted(k).nonzero()[0].tolist() == [slot]
        assert pv.told.admitted(k).nonzero()[0].tolist() == ([m["target"]] if m["line"] is not None else [])
        if m["line"] is None:
            assert not pv.told.variant_sizes[k].any() and not pv.told.write_counts[k].any()
    assert pv.line(0) == b"~OLFive asks you:~RS ~FRred~RS hello?\n" and pv.line(1) == b"~OL>>~RS A presence waves\n"
    assert pv.reply_text(3) == b"Thirty is AFK, message is: ~FRaway\n" and pv.line(5) == b"~OL>>~RS Five me\n"
    told, reply = pv.told.expand(), pv.reply.expand()                   # both plans expand into ordinary fan-outs
    cap = pv.told.capacity
    assert told.admitted.nonzero()[0].tolist() == [0 * cap + 66, 1 * cap + 5, 5 * cap + 5]
    assert reply.admitted.nonzero()[0].tolist() == [kk * cap + e[0] for kk, e in enumerate(events)]
    assert told.output(told.item(0, 66)) == nuts_path.transduce(models[0]["line"], int(colour[66])) and colour[66]
    assert reply.output(reply.item(0, 5)) == nuts_path.transduce(models[0]["reply"], int(colour[5]))
    for bad_k in (-1, 8):
        with pytest.raises(IndexError):
            pv.line(bad_k)
        with pytest.raises(IndexError):
            pv.reply_text(bad_k)


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def tell_run(built):
    res = child_run.run_child("device_tell_child.py", "DEVICE_TELL", 600)
    print("\n[tell]", json.dumps(res)[:4000])
    return res


@pytest.mark.gpu
def test_the_golden_sessions_replay_on_the_device(tell_run):
    g = tell_run["golden"]
    assert list(g) == list(GOLDEN)
    for name in GOLDEN:
        assert g[name]["private_steps"] == GOLDEN_PRIVATE_STEPS[name], name
        assert g[name]["comparisons"] == GOLDEN_COMPARISONS[name], name
        assert g[name]["mismatches"] == [] and g[name]["n_bad_vs_model"] == 0, (name, g[name])
    assert sum(g[name]["private_steps"] for name in GOLDEN) == 38


@pytest.mark.gpu
def test_seeded_events_match_the_model(tell_run):
    f = tell_run["fuzz"]
    assert f["capacities"] == list(CAPACITIES) == [1, 63, 64, 65, 255, 256, 257, 1000]
    assert f["calls"] == 2 * len(CAPACITIES) and f["events"] == f["calls"] * EVENTS_PER_CALL and EVENTS_PER_CALL == 300
    assert f["longest_inpstr"] == 999
    by = f["outcome_by_com"]
    for outcome in OUTCOMES:
        for com in COMS:
            assert by.get(f"{outcome}/{com}", 0) > 0, (outcome, com, by)
    assert {0, 63, 64, 255, 256, 999} <= set(f["targets"])              # and capacity - 1 of the others:
    assert {62, 254, 256} <= set(f["targets"])
    assert {0, 1, 12, 13, 39} <= set(f["word_lengths"]) and max(f["word_lengths"]) == 39
    assert f["self_by_substring"] > 0                                   # a pemote that went to its speaker
    assert f["n_bad"] == 0, f["first_bad"]


@pytest.mark.gpu
def test_both_plans_are_plan_many_of_the_composed_texts(tell_run):
    c = tell_run["contract"]
    assert c["checked"] >= 40 and c["coms"] == sorted(COMS) and c["void"] >= 40
    assert c["n_bad"] == 0, c["first_bad"]


@pytest.mark.gpu
def test_recording_told_lines_into_the_revtell_rings(tell_run):
    r = tell_run["recording"]
    assert r["tell_calls"] >= 9 and r["clears"] >= 2 and r["reviews"] >= 7
    assert r["recorded"] > 200 and r["lines_compared"] > 50 and r["most_to_one_target_in_one_call"] > 64
    assert r["n_bad"] == 0, r["first_bad"]
    assert r["same_on_a_second_run"] is True


@pytest.mark.gpu
def test_nothing_else_moved(tell_run):
    m = tell_run["moved"]
    for later in ("after_telling", "after_telling_twice", "after_private_update", "after_telling_again"):
        assert m[later] == m["fresh"], later                            # results and copy volumes alike
    assert m["private_update_left_dirty"] == [False, False, False, False]
    h, cap = m["tell_h2d"], m["capacity"]
    assert len(set(h["clean"])) == 1 and len(m["tell_d2h"]) == 1        # the copies depend on the events alone
    assert 80 * cap <= h["after_private_update"] - h["clean"][0] < 80 * cap + 512       # speaker state and AFK messages
    assert 64 * cap <= h["after_afk_mesg_update"] - h["clean"][0] < 64 * cap + 256      # the AFK messages alone
