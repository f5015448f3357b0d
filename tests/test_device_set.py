"""``Roster.set_many``: the fourteen commands a user sets its own state with, decided and composed on the device
(nuts_roster_set and nuts_roster_set_order of fanout.hip), and ``device.Settings``.

Host tier (unmarked): the new names; everything malformed is rejected before the device library loads, and a rejected call
changes no mirror and no dirty flag; the Python model of the twelve functions (``setting`` and ``set_call`` of
tests/device_set_child.py) reproduces every such step of the new recording and of the eight replay sessions through
``SetReplayer``, the actor's own bytes included; the new recording holds every outcome; the deferral rule on hand-built
event lists; over a library that computes nothing, ``set_many`` is passed exactly the mirrors whose flags were set, applies
the result in event order and leaves everything unchanged after a rejected call; ``update(prompt=, charmode_echo=)`` alone
makes no other call upload; the longest texts stay within their rows.

GPU tier: everything that touches the device runs in ONE short-lived child for the module (tests/device_set_child.py,
under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

import child_run
import session_replay as sr
from device_rooms_child import list_room
from device_set_child import (CAPACITIES, EDGE_SLOTS, EVENTS, NAMES, SESSIONS, WAS_TRACKED, SetReplayer, deliveries, fuzz_part, load,
                              mirror_differences, seat, set_call, set_list_rooms, set_user, setting)
from nuts333_amd import device, nuts_path
from test_device_go import FakeLibrary, mirrors, passed

REPO = Path(__file__).resolve().parent.parent
G = device
FLAGS = ("_dirty", "_speech_dirty", "_private_dirty", "_set_dirty", "_afk_dirty", "_rooms_dirty", "_udesc_dirty", "_who_dirty",
         "_clones_dirty", "_go_dirty")
(MODE, IGNALL, PROMPT, DESC, INPHR, OUTPHR, TOPIC, VIS, INVIS, CHARECHO, AFK, COLOUR, IGNSHOUT, IGNTELL) = G.SET_COMS


def flags(r):
    return tuple(getattr(r, f) for f in FLAGS)


def only(*names):
    return tuple(f in names for f in FLAGS)


def clean(r):
    for f in FLAGS:
        setattr(r, f, False)


def hand_rooms() -> list:
    return [list_room(b"den", links=[1], topic=b"tea at four"), list_room(b"hall", links=[0])]


def hand_users() -> dict:
    return {0: set_user(0, name=b"Alice", room=0, colour=1), 1: set_user(1, name=b"Bobby", room=0), 2: set_user(2, name=b"Carol", room=0, ignall=1),
            3: set_user(3, name=b"Dave", room=1, level=3, vis=0, afk_mesg=b"kept"), 4: set_user(4, name=b"Erica", room=7),
            5: set_user(5, name=None, room=0), 6: set_user(6, name=b"Prompt", room=0, login=1), 7: set_user(7, name=None, room=None)}


def seated(capacity=8, **kw):
    rms, users = hand_rooms(), hand_users()
    r = device.Roster(capacity, look_rooms=len(rms), **kw)
    set_list_rooms(r, rms)
    seat(r, {j: u for j, u in users.items() if u["room"] is not None})
    return r, users, rms


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


# ------------------------------------------------------------------ host tier: names and input checks
OUTCOME_NAMES = ("MODE_COMMAND", "MODE_SPEECH", "IGNALL_ON", "IGNALL_OFF", "PROMPT_ON", "PROMPT_OFF", "DESC_SET", "INPHR_SET", "OUTPHR_SET",
                 "TOPIC_SET", "VISIBLE", "INVISIBLE", "CHARECHO_ON", "CHARECHO_OFF", "AFK", "AFK_LOCKED", "COLOUR_ON", "COLOUR_OFF", "IGNSHOUT_ON",
                 "IGNSHOUT_OFF", "IGNTELL_ON", "IGNTELL_OFF", "COLOUR_TEST", "DESC_QUERY", "DESC_CLONE", "DESC_LONG", "PHRASE_LONG", "INPHR_QUERY",
                 "OUTPHR_QUERY", "TOPIC_NONE", "TOPIC_QUERY", "TOPIC_LONG", "ALREADY_VISIBLE", "ALREADY_INVISIBLE", "AFK_LONG", "DEFERRED")


def test_the_new_names_exist():
    # the numbers are enum np_com's, what a COMMAND read of input_many hands back
    assert {n: nuts_path.lib().np_command_name(c).decode() for n, c in NAMES.items()} == {n: n for n in NAMES} and len(NAMES) == 14
    assert (G.COM_MODE, G.COM_IGNALL, G.COM_PROMPT, G.COM_DESC, G.COM_INPHR, G.COM_OUTPHR, G.COM_TOPIC, G.COM_VIS, G.COM_INVIS,
            G.COM_CHARECHO) == (2, 11, 12, 13, 14, 15, 20, 55, 56, 66)
    assert G.SET_COMS == tuple(NAMES.values()) and G.SET_KERNELS == ("nuts_roster_set", "nuts_roster_set_order")
    assert not set(G.SET_KERNELS) & (set(G.KERNELS) | set(G.WHO_KERNELS) | set(G.ROOMS_KERNELS) | set(G.GO_KERNELS) | set(G.ACCESS_KERNELS)
                                     | set(G.CLONE_KERNELS))
    source = device.SOURCE.read_text()
    assert "nuts_roster_set(SetArgs a)" in source and "nuts_roster_set_order(SetOrderArgs a)" in source and "int nd_roster_set(" in source
    assert [getattr(G, "SET_" + n) for n in OUTCOME_NAMES] == list(range(36))
    for n in OUTCOME_NAMES:                                             # the kernel's constants, by the same names and numbers
        assert f"kSet{n.title().replace('_', '')} = {getattr(G, 'SET_' + n)}" in source, n
    for n, c in NAMES.items():
        assert f"kCom{n.title()} = {c}" in source, n
    assert (G.MAX_SET_HERE, G.MAX_SET_REPLY, G.MAX_SET_REPLY2) == (96, 83, 17) and G._SET_ROWS == (96, 84, 20)
    assert "constexpr int kSetHereRow = 96, kSetReplyRow = 84, kSetReply2Row = 20;" in source
    assert "kSetHereMax == 96 && kSetReplyMax == 83 && kSetReply2Max == 17" in source
    assert (G.SET_HERE, G.SET_REPLY, G.SET_REPLY2) == (0, 1, 2)
    assert G.SET_FLAGS == {"prompt": 32, "charmode_echo": 64} and "kPrompt = 32, kCharecho = 64" in source
    assert not set(G.SET_FLAGS.values()) & set(G.SPEECH_FLAGS.values())
    assert callable(G.Roster.set_many) and G.Settings.__dataclass_fields__.keys() >= {
        "outcome", "reply", "reply2", "here", "reply_colour", "texts", "text_starts", "text_sizes", "timing"}
    assert len(G.COLOUR_TEST) == 20 and G.COLOUR_TEST[0] == b"OL: ~OLNUTS 3 VIDEO TEST~RS\n" and G.COLOUR_TEST[-1] == b"BW: ~BWNUTS 3 VIDEO TEST~RS\n"
    doc = G.Roster.set_many.__doc__
    assert all(word in doc for word in ("the prompt", "nuts333.c:180-203", "remote users", "home execution", "relay_many", "level check",
                                        "SET_DEFERRED", "SET_COLOUR_TEST"))
    assert "reply_colour" in G.Settings.__doc__ and "not by\n    ``reply.colour_bits``" in G.Settings.__doc__
    assert "set_many" in G.__doc__


@pytest.mark.parametrize("events, why", [
    ([], "empty call"), ((), "empty call"), (None, "events must be a sequence"), ("x", "events must be a sequence"),
    ([(0, b"", 1)], "event 0: expected a \\(slot, com, inpstr, word_count\\) tuple"), ([[0, DESC, b"", 1]], "event 0: expected"),
    ([(0, DESC, b"", 1), (8, DESC, b"", 1)], "event 1: slot"), ([(True, DESC, b"", 1)], "event 0: slot"),
    ([(0, 3, b"", 1)], "event 0: com must be"), ([(0, 87, b"", 1)], "event 0: com must be"), ([(0, G.COM_GO, b"den", 2)], "event 0: com must be"),
    ([(0, True, b"", 1)], "event 0: com must be"), ([(0, None, b"", 1)], "event 0: com must be"), ([(0, 92, b"", 1)], "event 0: com must be"),
    ([(0, DESC, 5, 2)], "event 0: inpstr|event 0: text"), ([(0, DESC, b"a\0b", 2)], "event 0: text contains a NUL"),
    ([(0, AFK, b"x" * 1000, 2)], "event 0: inpstr of 1000 bytes"), ([(0, AFK, b"brb", 11)], "event 0: word_count"),
    ([(0, AFK, b"brb", -1)], "event 0: word_count"), ([(0, AFK, b"brb", None)], "event 0: word_count"),
    ([(0, VIS, b"", 1), (5, VIS, b"", 1)], "event 1: the actor, slot 5, has no name"),
    ([(6, VIS, b"", 1)], "event 0: the actor, slot 6, is still logging in"), ([(7, VIS, b"", 1)], "event 0: the actor, slot 7, is in no room"),
    ([(4, TOPIC, b"", 1)], "event 0: a .topic by slot 4 in room 7, which has no room record"),
])
def test_malformed_events_are_rejected_before_the_library_loads(no_library, events, why):
    r, _, _ = seated()
    clean(r)
    before = mirrors(r)
    with pytest.raises(ValueError, match=why):
        r.set_many(events)
    assert flags(r) == (False,) * len(FLAGS) and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))


def test_a_roster_without_rooms_a_closed_one_and_a_call_past_the_cap(no_library, monkeypatch):
    r = device.Roster(4)
    r.update(0, room=0, name=b"Alice")
    with pytest.raises(ValueError, match=r"event 0: a \.topic by slot 0 in room 0, which has no room record \(look_rooms is 0\)"):
        r.set_many([(0, TOPIC, b"", 1)])
    r, _, _ = seated()
    state, before = flags(r), mirrors(r)
    bound = 12 * 200 * 2 + 16 * 6
    monkeypatch.setattr(device, "MANY_ARENA_CAP", bound - 1)
    with pytest.raises(ValueError, match=f"call too large: its variant bound is {bound} bytes.*MANY_ARENA_CAP.*split it"):
        r.set_many([(0, VIS, b"", 1), (0, INVIS, b"", 1)])
    monkeypatch.undo()
    big = device.Roster(G.MAX_CAPACITY)
    big.update(0, room=0, name=b"Alice")
    monkeypatch.setattr(device, "_load", lambda: pytest.fail("loaded"))
    with pytest.raises(ValueError, match="K x capacity must be below"):
        big.set_many([(0, VIS, b"", 1)] * 32768)
    assert flags(r) == state and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))
    r.close()
    with pytest.raises(ValueError, match="closed"):
        r.set_many([(0, VIS, b"", 1)])


def test_the_thirteen_other_commands_need_no_room_records(fake):
    r = device.Roster(4)
    r.update(0, room=9, name=b"Alice")
    fake.set_script.append([(G.SET_ALREADY_VISIBLE, False)] * 13)
    r.set_many([(0, c, b"", 1) for c in G.SET_COMS if c != TOPIC])
    assert fake.calls[-1][0] == "nd_roster_set" and fake.calls[-1][1][14] is None


# ------------------------------------------------------------------ host tier: the model against the recordings
@pytest.fixture(scope="module")
def model_replays():
    return {name: (load(name), SetReplayer(load(name)).run()) for name in SESSIONS}


def test_the_model_reproduces_every_such_step_of_the_recorded_sessions(model_replays):
    were_tracked = 0
    for name, (doc, res) in model_replays.items():
        assert res["mismatches"] == [], (name, res["mismatches"][:1])
        assert res["set"] > 0 and res["plan_disagreements"] == 0 and res["comparisons"] > 0, name
        assert not set(res["commands"]) & set(WAS_TRACKED) or all(res["commands"][c] > 0 for c in set(res["commands"]) & set(WAS_TRACKED))
        if name != "set":                                               # sr.Replayer answers them too, now: the two agree step by step
            plain = sr.replay(doc)
            was = sum(plain["commands"].get(c, 0) for c in WAS_TRACKED)
            assert was == res["set"] and res["tracked"] == plain["tracked"] == 0 and res["answered"] == plain["answered"] == 60, name
            assert res["comparisons"] == plain["comparisons"]           # the actor's bytes of each, in both
            were_tracked += was
    assert [res["set"] for _, res in model_replays.values()] == [53, 6, 3, 2, 7, 1, 4, 4, 4] and were_tracked == 31


def test_what_the_new_recording_holds(model_replays):
    doc, res = model_replays["set"]
    assert [(a["level"], a["colour"]) for a in doc["accounts"][0]] == [(1, 1), (1, 0), (1, 0), (3, 1)]
    assert set(res["set_outcomes"]) == {str(o) for o in range(G.SET_DEFERRED)}, res["set_outcomes"]     # every outcome but DEFERRED
    assert 60 <= sum(1 for s in doc["steps"] if s["op"] == "line") <= 110 and res["returns"] == 7
    size = (REPO / "tests" / "golden" / "reference_only" / "set.json").stat().st_size
    assert size <= max(p.stat().st_size for p in (REPO / "tests" / "golden" / "reference_only").glob("*.json") if p.name != "set.json")
    by_note = {s["note"]: s for s in doc["steps"] if s.get("note")}
    mine = lambda note: by_note[note]["recv"][by_note[note]["actor"]]
    heard = lambda note, client: by_note[note]["recv"].get(client, "")
    assert mine("colour on by a user whose colour was off") == "Colour \x1b[32mON.\x1b[0m\n\r\x1b[0m"       # it arrives coloured
    assert mine("colour off") == "Colour \x1b[31mOFF.\x1b[0m\n\r\x1b[0m" and mine("the video test").count("NUTS 3 VIDEO TEST") == 20
    assert by_note["ignall by an invisible ARCH"]["recv"]["b"] == "Dave is now ignoring everyone.\n\r"   # the real name
    assert heard("ignall on", "c") == "" and heard("became invisible", "c") == "" and heard("ignall on", "b") != ""     # the listener who ignores everyone
    assert mine("vis when visible") == "You are already visible.\x1b[0m\n\r\x1b[0m" and "already invisible" in mine("invis when invisible")
    assert by_note["topic by an invisible actor"]["recv"]["b"] == "A presence has set the topic to: under the radar\n\r"
    assert heard("afk by an invisible user", "b") == "" and "AFK message set." in mine("afk with a message")
    assert by_note["afk"]["recv"]["b"] == "Alice goes AFK...\n\r" and by_note["afk lock"]["recv"]["b"] == "Alice goes AFK...\n\r"
    assert by_note["afk lock with a message"]["recv"]["b"] == "Alice goes AFK: back at ten\n\r"          # remove_first took the word off
    assert by_note["a word that is not lock"]["recv"]["b"] == "Alice goes AFK: lockx\n\r"
    for note in ("a 61-byte message", "a 61-byte message with lock"):
        assert "AFK message too long." in mine(note) and heard(note, "b") == ""
    assert "Description set." in mine("a desc of 30 bytes") and "Description too long." in mine("a desc of 31 bytes")
    assert by_note["(CLONE) inside the first word"]["send"] == ".desc the(CLONE)one" and "Description set." in mine("(CLONE) in the second word only")
    assert "a (CLONE)" in mine("desc query after")
    assert "In phrase set." in mine("an in phrase of 40 bytes") and "Phrase too long." in mine("an in phrase of 41 bytes")
    assert "Out phrase set." in mine("an out phrase of 40 bytes") and "Phrase too long." in mine("an out phrase of 41 bytes")
    assert len(by_note["a topic of 60 bytes"]["send"]) == 7 + 60 and "Topic too long." in mine("a topic of 61 bytes")
    assert "No topic has been set yet." in mine("topic query with no topic") and "The current topic is: " in mine("topic query")
    assert all(q in by_note for q in ("desc query", "inphr query", "outphr query"))


# ------------------------------------------------------------------ host tier: the deferral rule
def outcomes(call):
    return [e["outcome"] for e in call["events"]]


def test_the_same_actor_twice_is_deferred():
    users, rms = hand_users(), hand_rooms()
    call = set_call(users, rms, [(3, VIS, b"", 1), (3, AFK, b"", 1), (0, AFK, b"", 1)])
    assert outcomes(call) == [G.SET_VISIBLE, G.SET_DEFERRED, G.SET_AFK] and users[3]["vis"] == 1 and not users[3]["afk"]
    assert all(call["events"][1][kind] is None and call["events"][1]["plans"][kind] == [] for kind in ("here", "reply", "reply2"))
    again = set_call(users, rms, [(3, AFK, b"", 1)])                    # submitted again it is answered: a call of one never defers
    assert outcomes(again) == [G.SET_AFK] and again["events"][0]["here"] == b"Dave goes AFK: kept\n"
    # decided against the snapshot the invisible Dave would have sent no line: the rule is what keeps the device exact
    assert setting(hand_users(), hand_rooms(), 3, AFK, b"", 1)["here"] is None


def test_an_ignall_toggle_then_a_room_line_in_the_same_room_is_deferred_and_in_another_room_is_not():
    users, rms = hand_users(), hand_rooms()
    call = set_call(users, rms, [(2, IGNALL, b"", 1), (0, INVIS, b"", 1), (1, IGNSHOUT, b"", 1), (3, TOPIC, b"elsewhere", 2)])
    # Carol listens again; Alice's line in the same room waits; Bobby's toggle has no line; Dave stands in the hall
    assert outcomes(call) == [G.SET_IGNALL_OFF, G.SET_DEFERRED, G.SET_IGNSHOUT_ON, G.SET_TOPIC_SET]
    assert call["events"][0]["plans"]["here"] == [0, 1, 5] and call["events"][3]["plans"]["here"] == []
    again = set_call(users, rms, [(0, INVIS, b"", 1)])
    assert again["events"][0]["plans"]["here"] == [1, 2, 5]             # Carol hears it now
    users, rms = hand_users(), hand_rooms()
    call = set_call(users, rms, [(0, COLOUR, b"", 1), (1, VIS, b"", 1), (1, INVIS, b"", 1)])
    assert outcomes(call) == [G.SET_COLOUR_OFF, G.SET_ALREADY_VISIBLE, G.SET_DEFERRED]      # a colour toggle counts; a refusal has no line


def test_a_refusal_and_a_query_defer_nothing():
    users, rms = hand_users(), hand_rooms()
    events = [(0, VIS, b"", 1), (0, DESC, b"", 1), (0, DESC, b"d" * 31, 2), (0, TOPIC, b"", 1), (0, AFK, b"m" * 61, 2), (0, INPHR, b"", 1), (0, IGNALL, b"", 1)]
    call = set_call(users, rms, events)
    assert outcomes(call) == [G.SET_ALREADY_VISIBLE, G.SET_DESC_QUERY, G.SET_DESC_LONG, G.SET_TOPIC_QUERY, G.SET_AFK_LONG, G.SET_INPHR_QUERY,
                              G.SET_IGNALL_ON]
    assert call["events"][3]["reply"] == b"The current topic is: tea at four\n"


def test_two_topics_of_one_room():
    users, rms = hand_users(), hand_rooms()
    call = set_call(users, rms, [(0, TOPIC, b"first", 2), (1, TOPIC, b"", 1), (1, TOPIC, b"second", 2), (3, TOPIC, b"", 1), (1, DESC, b"", 1)])
    assert outcomes(call) == [G.SET_TOPIC_SET, G.SET_DEFERRED, G.SET_DEFERRED, G.SET_TOPIC_NONE, G.SET_DESC_QUERY] and rms[0]["topic"] == b"first"
    assert outcomes(set_call(users, rms, [(1, TOPIC, b"", 1)])) == [G.SET_TOPIC_QUERY]


def test_the_decision_chain_of_one_event():
    users, rms = hand_users(), hand_rooms()
    one = lambda slot, com, inpstr=b"", wc=None: setting(users, rms, slot, com, inpstr, (1 + len(sr.words_of(inpstr))) if wc is None else wc)
    assert one(0, DESC, b"x", 1)["outcome"] == G.SET_DESC_QUERY         # word_count decides, not the words
    assert one(0, DESC, b"a(CLONE)")["outcome"] == G.SET_DESC_CLONE and one(0, DESC, b"a (CLONE)")["outcome"] == G.SET_DESC_SET
    assert one(0, DESC, b"(CLONE) " + b"d" * 40)["outcome"] == G.SET_DESC_CLONE            # before the length
    assert one(0, DESC, b"w" * 39 + b"(CLONE)")["outcome"] == G.SET_DESC_LONG              # word[1] is cut at 39 bytes
    assert one(0, DESC, b"w" * 33 + b"(CLONE)")["outcome"] == G.SET_DESC_LONG and one(0, DESC, b"w" * 32 + b"(CLONE)")["outcome"] == G.SET_DESC_CLONE
    assert one(0, INPHR, b"p" * 41, 1)["outcome"] == G.SET_PHRASE_LONG and one(0, OUTPHR, b"p" * 40, 1)["outcome"] == G.SET_OUTPHR_QUERY
    assert one(0, OUTPHR, b"p" * 40)["change"] == {"out_phrase": b"p" * 40}
    assert one(3, TOPIC, b"t" * 61)["outcome"] == G.SET_TOPIC_LONG and one(3, TOPIC, b"t" * 60)["here"] == b"A presence has set the topic to: " + b"t" * 60 + b"\n"
    assert one(0, AFK, b"lock")["outcome"] == G.SET_AFK_LOCKED and one(0, AFK, b"lock")["reply2"] is None
    got = one(0, AFK, b"  lock   gone  fishing ")
    assert (got["outcome"], got["change"], got["here"]) == (G.SET_AFK_LOCKED, {"afk": 2, "afk_mesg": b"gone  fishing "}, b"Alice goes AFK: gone  fishing \n")
    assert one(0, AFK, b"Lock up")["change"] == {"afk": 1, "afk_mesg": b"Lock up"} and one(0, AFK, b"lock " + b"m" * 61)["outcome"] == G.SET_AFK_LONG
    assert one(0, AFK, b"lock " + b"m" * 60)["outcome"] == G.SET_AFK_LOCKED and one(0, AFK, b"m" * 57 + b" brb")["outcome"] == G.SET_AFK_LONG
    assert one(0, AFK, b"brb", 1)["reply2"] is None and one(0, AFK, b"brb", 1)["here"] == b"Alice goes AFK...\n"
    assert one(3, AFK, b"brb")["here"] is None and one(3, AFK, b"brb")["reply2"] == b"AFK message set.\n"
    users[0].update(command_mode=1, ignall=1, charmode_echo=1)
    assert one(0, COLOUR)["outcome"] == G.SET_COLOUR_TEST and one(0, COLOUR)["reply"] is None and one(0, COLOUR)["change"] == {}
    users[0].update(charmode_echo=0)
    assert (one(0, COLOUR)["outcome"], one(0, COLOUR)["reply_colour"]) == (G.SET_COLOUR_OFF, 1)
    assert (one(1, COLOUR)["outcome"], one(1, COLOUR)["reply_colour"], one(1, VIS)["reply_colour"]) == (G.SET_COLOUR_ON, 1, 0)


def test_deliveries_follow_the_call_order_and_the_colour_of_the_moment():
    users, rms = hand_users(), hand_rooms()
    before = {j: dict(u) for j, u in users.items()}
    call = set_call(users, rms, [(0, AFK, b"~FRtea", 2), (1, COLOUR, b"", 1), (1, IGNSHOUT, b"", 1)])
    assert outcomes(call) == [G.SET_AFK, G.SET_COLOUR_ON, G.SET_DEFERRED]
    out = deliveries(before, call)
    assert out[1] == nuts_path.transduce(b"Alice goes AFK: ~FRtea\n", 0) + nuts_path.transduce(b"Colour ~FGON.\n", 1)
    assert out[0] == b"".join(nuts_path.transduce(t, 1) for t in (b"You are now AFK, press <return> to reset.\n", b"AFK message set.\n"))
    assert out[2] == b"" and out[5] == nuts_path.transduce(b"Alice goes AFK: ~FRtea\n", 0)


# ------------------------------------------------------------------ host tier: the bounds
def test_the_longest_texts_stay_within_their_rows():
    rms = [list_room(b"den", topic=b"\n" * 60)]
    users = {0: set_user(0, name=b"\n" * 12, room=0, desc=b"\n" * 30, in_phrase=b"\n" * 40, out_phrase=b"\n" * 40, afk_mesg=b"\n" * 60),
             1: set_user(1, name=b"I" * 12, room=0, vis=0)}
    longest = {"here": 0, "reply": 0, "reply2": 0}
    events = [(0, c, b"", 1) for c in G.SET_COMS] + [(0, TOPIC, b"\n" * 60, 2), (0, AFK, b"\n" * 60, 2), (0, AFK, b"lock " + b"\n" * 60, 3),
                                                      (0, INVIS, b"", 1), (1, VIS, b"", 1), (1, TOPIC, b"t" * 60, 2), (0, DESC, b"d" * 30, 2)]
    for slot, com, inpstr, wc in events:
        res = setting(users, rms, slot, com, inpstr, wc)
        for kind, most, row in zip(longest, (G.MAX_SET_HERE, G.MAX_SET_REPLY, G.MAX_SET_REPLY2), G._SET_ROWS):
            text = res[kind]
            if text is None:
                continue
            longest[kind] = max(longest[kind], len(text))
            assert len(text) <= most <= row
            for c in (0, 1):
                ch = nuts_path.chunks(text, c)
                assert sum(map(len, ch)) <= device.max_bytes(most) and len(ch) <= device.MAX_WRITES
    assert longest == {"here": 96, "reply": 83, "reply2": 17}


def test_the_seeded_stream_of_the_model_holds_every_outcome():
    f = fuzz_part(20263, on_device=False)                               # the child's default seed
    assert set(f["outcomes"]) == {str(o) for o in range(36)}, f["outcomes"]
    assert f["colours"] == [0, 1] and f["edge_slots"] == list(EDGE_SLOTS)


# ------------------------------------------------------------------ the apply step, over a library that computes nothing
SET_MIRROR_ARGS = {9: "_table", 10: "_speech", 11: "_afk", 12: "_udesc", 13: "_go", 14: "_rooms"}


class SetFakeLibrary(FakeLibrary):
    """The go tests' library that computes nothing; ``nd_roster_set`` answers with the next entry of ``set_script``: per
    event ``(outcome, whether it has a second reply)``."""

    def __init__(self, arrays: dict):
        super().__init__(arrays)
        self.set_script = []

    def __getattr__(self, name):
        call = super().__getattr__(name)
        if name != "nd_roster_set":
            return call

        def set_(*args):
            call(*args)
            answer = self.set_script.pop(0)
            self.arrays[args[15]][:] = [e[0] for e in answer]
            self.arrays[args[16]][:] = -1
            self.arrays[args[16]][G.SET_REPLY2, [k for k, e in enumerate(answer) if e[1]]] = 17
            for at in (18, 19):
                self.arrays[args[at]][:] = 0
            return 0
        return set_


@pytest.fixture
def fake(monkeypatch):
    arrays: dict = {}
    lib = SetFakeLibrary(arrays)
    real = device._ptr

    def ptr(a):
        arrays[a.ctypes.data] = a
        return real(a)

    monkeypatch.setattr(device, "_ptr", ptr)
    monkeypatch.setattr(device, "_load", lambda: lib)
    return lib


def scripted(lib, users, rms, events):
    call = set_call(users, rms, events)
    lib.set_script.append([(e["outcome"], e["reply2"] is not None) for e in call["events"]])
    return call


def test_set_many_is_passed_exactly_the_dirty_mirrors_and_applies_the_result_in_event_order(fake):
    r, users, rms = seated()
    users = {j: u for j, u in users.items() if u["room"] is not None}
    scripted(fake, users, rms, [(0, DESC, b"", 1)])
    got = r.set_many([(0, DESC, b"", 1)])
    name, args = fake.calls[-1]
    assert name == "nd_roster_set" and args[1] == 1 and len(args) == 24
    assert all(args[i] == getattr(r, m).ctypes.data for i, m in SET_MIRROR_ARGS.items() if m != "_rooms") and args[14] is None
    assert flags(r) == only("_rooms_dirty", "_who_dirty", "_clones_dirty") and got.effective().tolist() == [] and len(fake.calls) == 1
    scripted(fake, users, rms, [(0, TOPIC, b"", 1)])                    # the room table travels with the first .topic
    r.set_many([(0, TOPIC, b"", 1)])
    assert passed(fake, r) == {"_rooms"} and flags(r) == only("_who_dirty", "_clones_dirty")
    for fields, want in (({"invite_room": 1}, {"_go"}), ({"room": 1}, {"_table"}), ({"level": 1}, {"_speech"}), ({"desc": b"d"}, {"_udesc"}),
                         ({"afk_mesg": b"brb"}, {"_afk"}), ({"afk": 1}, {"_speech"}), ({"prompt": 1}, {"_speech"}), ({"last_login": 4}, set())):
        r.update(4, **fields)
        scripted(fake, users, rms, [(0, VIS, b"", 1)])
        r.set_many([(0, VIS, b"", 1)])
        assert passed(fake, r) == want, fields
        assert not (r._speech_dirty or r._private_dirty or r._set_dirty)
    r.update(4, room=7, afk=0, prompt=0)
    users[4].update(desc=b"d", afk_mesg=b"brb")
    r.set_rooms(1, topic=b"t")
    scripted(fake, users, rms, [(0, VIS, b"", 1)])
    r.set_many([(0, VIS, b"", 1)])
    assert "_rooms" not in passed(fake, r) and r._rooms_dirty              # no .topic in the call: the room table stays behind
    rms[1]["topic"] = b"t"
    scripted(fake, users, rms, [(3, TOPIC, b"", 1)])
    r.set_many([(3, TOPIC, b"", 1)])
    assert passed(fake, r) == {"_rooms"} and not r._rooms_dirty
    # one call of every kind of change, applied in event order; the deferred one changes nothing
    events = [(0, IGNALL, b"", 1), (1, DESC, b"sips tea", 3), (1, AFK, b"never", 2), (3, TOPIC, b"under the radar", 4), (3, AFK, b"lock away now", 4),
              (4, INPHR, b"tiptoes in", 3), (2, COLOUR, b"", 1), (2, OUTPHR, b"x", 2)]
    call = scripted(fake, users, rms, events)
    got = r.set_many(events)
    assert outcomes(call) == got.outcome.tolist() == [G.SET_IGNALL_ON, G.SET_DESC_SET, G.SET_DEFERRED, G.SET_TOPIC_SET, G.SET_DEFERRED,
                                                      G.SET_INPHR_SET, G.SET_COLOUR_ON, G.SET_DEFERRED]
    assert got.effective().tolist() == [0, 1, 3, 5, 6] and got.reply_colour.tolist() == [1, 0, 0, 0, 0, 0, 1, 0]
    assert mirror_differences(r, users, rms) == [] and users[1]["afk"] == 0 and users[3]["afk_mesg"] == b"kept"
    assert flags(r) == only("_dirty", "_udesc_dirty", "_rooms_dirty", "_go_dirty", "_who_dirty", "_clones_dirty")
    again = [(1, AFK, b"never", 2), (3, AFK, b"lock away now", 4), (2, OUTPHR, b"x", 2), (0, MODE, b"", 1), (4, PROMPT, b"", 1), (4, CHARECHO, b"", 1)]
    call = scripted(fake, users, rms, again)
    got = r.set_many(again)
    assert passed(fake, r) == {"_table", "_udesc", "_go"} and got.outcome.tolist() == outcomes(call)
    assert outcomes(call) == [G.SET_AFK, G.SET_AFK_LOCKED, G.SET_OUTPHR_SET, G.SET_MODE_COMMAND, G.SET_PROMPT_ON, G.SET_DEFERRED]
    assert mirror_differences(r, users, rms) == [] and bytes(r._afk[3, :8]) == b"away now" and users[3]["afk"] == 2
    assert flags(r) == only("_speech_dirty", "_private_dirty", "_set_dirty", "_afk_dirty", "_go_dirty", "_who_dirty", "_clones_dirty",
                            "_rooms_dirty")                             # the topic set before: no .topic since, so it still waits
    # the calls that follow are passed what changed: tell_many the speaker mirror and the messages, go_many the go mirror
    r.tell_many([(0, G.COM_TELL, b"bobby hi", 3)])
    assert fake.calls[-1][0] == "nd_roster_tell" and passed(fake, r) == {"_speech", "_afk"}
    assert flags(r) == only("_set_dirty", "_go_dirty", "_who_dirty", "_clones_dirty", "_rooms_dirty")


def test_a_rejected_call_changes_nothing_after_an_accepted_one(fake):
    r, users, rms = seated()
    users = {j: u for j, u in users.items() if u["room"] is not None}
    scripted(fake, users, rms, [(1, IGNALL, b"", 1)])
    r.set_many([(1, IGNALL, b"", 1)])
    state, before, calls = flags(r), mirrors(r), len(fake.calls)
    with pytest.raises(ValueError, match="event 1: com must be"):
        r.set_many([(1, IGNALL, b"", 1), (1, 99, b"", 1)])
    assert flags(r) == state and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before)) and len(fake.calls) == calls


def test_an_update_of_prompt_and_charmode_echo_alone_makes_no_other_call_upload(fake):
    r, users, rms = seated(review_rooms=2, revtell=True, clones=1)
    r.update(4, room=1)
    clean(r)
    r.update([0, 1], prompt=1, charmode_echo=[0, 1])
    assert flags(r) == only("_set_dirty") and r._speech[1, G.USER_NAME_LEN + 1] == 1 | 32 | 64 and r._speech[0, G.USER_NAME_LEN + 1] == 1 | 32
    with pytest.raises(ValueError, match="prompt"):
        r.update(0, prompt=2)
    fake.script.append([(G.GO_WHERE, -1, 0, 0)])
    calls = (lambda: r.speak_many([(0, G.COM_SAY, b"hi", 1)]), lambda: r.input_many([(0, b"hi\n")]), lambda: r.tell_many([(0, G.COM_TELL, b"bobby hi", 3)]),
             lambda: r.look_many([0]), lambda: r.who_many([0], now=1, date=b"D"), lambda: r.rooms_many([0], topics=True),
             lambda: r.go_many([(0, b"", 1)], gatecrash_level=3, min_private_users=2), lambda: r.plan_many([(b"x\n", 0, None, 0, G.COM_SAY)]),
             lambda: r.relay_many([(b"x\n", 0, None, 0, G.COM_SAY)]))
    for call in calls:
        call()
        assert passed(fake, r) == set() and r._set_dirty, fake.calls[-1][0]
    fake.set_script.append([(G.SET_ALREADY_VISIBLE, False)])
    r.set_many([(0, VIS, b"", 1)])
    assert passed(fake, r) == {"_speech"} and flags(r) == (False,) * len(FLAGS)


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def set_run(built):
    res = child_run.run_child("device_set_child.py", "DEVICE_SET", 300)
    print("\n[set]", json.dumps(res)[:6000])
    return res


@pytest.mark.gpu
def test_the_recorded_sessions_replay_on_the_device(set_run, model_replays):
    g = set_run["golden"]
    assert sorted(g) == sorted(["set:compact", "set:spread"] + [f"{name}:compact" for name in SESSIONS[1:]])
    for key, part in g.items():
        doc, model = model_replays[key.split(":")[0]]
        assert part["n_mismatches"] == 0, (key, part["mismatches"])
        assert part["set"] == part["calls"] == model["set"] and part["returns"] == model["returns"], key
        assert part["outcomes"] == model["set_outcomes"] and part["plan_disagreements"] == 0, key
        assert part["comparisons"] == model["comparisons"] and part["capacity"] >= (257 if key.endswith(sr.SPREAD) else 8)


@pytest.mark.gpu
def test_seeded_streams_match_the_model(set_run):
    f = set_run["fuzz"]
    assert f["capacities"] == list(CAPACITIES) == [1, 8, 63, 64, 65, 257] and f["events_per_call"] == list(EVENTS) == [1, 3, 4, 5, 64, 65]
    assert f["events"] == len(CAPACITIES) * sum(EVENTS) and f["calls"] > len(CAPACITIES) * len(EVENTS)      # the deferred ones again
    assert set(f["outcomes"]) == {str(o) for o in range(36)}, f["outcomes"]     # every outcome, SET_DEFERRED among them
    assert f["colours"] == [0, 1] and f["edge_slots"] == [0, 63, 64, 256]
    assert f["n_bad"] == 0, f["first_bad"]


@pytest.mark.gpu
def test_the_edges(set_run):
    e = set_run["edges"]
    assert e["n_bad"] == 0, e["first_bad"]
    assert e["twelve"] == [G.SET_IGNALL_ON, G.SET_TOPIC_SET] and e["twelve_here"] == "Abcdefghijkl is listening again.\n" and e["twelve_to"] == [6, 63]
    assert e["longest"] == [G.SET_DESC_LONG, G.SET_PHRASE_LONG, G.SET_TOPIC_LONG, G.SET_AFK_LONG]
    assert e["alone"] == [G.SET_INVISIBLE, G.SET_ALREADY_VISIBLE]
    assert e["kept"] == [G.SET_AFK] and e["kept_lock"] == [G.SET_AFK_LOCKED]
    # the actor alone in its room: the line is planned, both variants are there, and nobody is admitted
    assert e["kept_here"] == "Twelve_bytes goes AFK: kept from before\n" and e["kept_to"] == []
    assert e["kept_sizes"] == [[len(e["kept_here"]) + 1, len(e["kept_here"]) + 1 + 8], [1, 2]]


@pytest.mark.gpu
def test_the_calls_that_follow_see_the_new_state(set_run):
    f = set_run["following"]
    assert f["n_bad"] == 0, f["first_bad"]
    assert f["leave"] == "Carol tiptoes to the hall.\n"


@pytest.mark.gpu
def test_a_second_run_gives_identical_bytes(set_run):
    assert set_run["determinism"] == {"same_on_a_second_call": True, "same_on_a_second_roster": True}


@pytest.mark.gpu
def test_set_many_meets_a_regrown_allocation(set_run):
    g = set_run["regrown"]
    assert g["small_outcome"] == G.SET_DESC_QUERY and g["clean_before"] and g["n_bad"] == 0, g
    assert g["big_h2d"] >= 5 * g["capacity"] + 600 * 4 and g["small_h2d"] < g["big_h2d"]


@pytest.mark.gpu
def test_the_child_stays_quick(set_run):
    assert sum(set_run["seconds"].values()) < 60, set_run["seconds"]
