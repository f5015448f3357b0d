"""``Roster.act_many``: ``.move``, ``.wake``, ``.muzzle`` and ``.unmuzzle`` decided and composed on the device
(nuts_roster_act and nuts_roster_act_order of fanout.hip), ``device.Act``, and ``Roster.update(muzzle_level=)``.

Host tier (unmarked): the names, numbers and row widths agree with the source text; everything malformed is rejected
before the device library loads, and a rejected call changes no mirror and no dirty flag; ``update(muzzle_level=)`` sets
byte 15, the bit and the dirty flag; the decision chain of the Python model of ``move()``, ``wake()``, ``muzzle()`` and
``unmuzzle()`` (``act`` and ``act_call`` of tests/device_act_child.py) on hand-built states, and the deferral rule key by
key; over a library that computes nothing, ``act_many`` is passed exactly the mirrors whose flags were set and leaves the
mirrors as the model's state, and a following ``speak_many`` and ``look_many`` are passed the tables that changed; the
longest texts stay within their rows.

GPU tier: everything that touches the device runs in ONE short-lived child for the module (tests/device_act_child.py,
under ``timeout``), and the tests assert on its JSON.  ``python tests/device_act_child.py --profile
profiles/device_act_mi355xhost.json`` keeps the parts' seconds.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import child_run
import session_replay as sr
from device_act_child import (EDGE_SLOTS, GET_USER_WORDS, KINDS, SESSIONS, ActReplayer, act, act_call, act_lines, act_user, cases,
                              fuzz_part, load, muzzle_of, seat_all)
from device_go_child import ARCH, CAPACITIES, EVENTS, LOOK_ROOMS, WIZ, seat_clones, set_rooms
from device_rooms_child import list_room
from nuts333_amd import device, nuts_path
from test_device_go import FLAGS, FakeLibrary, clean, flags, mirrors, model_state_differences, only, passed

G = device
GOD = G.MAX_LEVEL
KW = {"gatecrash_level": ARCH, "min_private_users": 2}
MOVE, WAKE, MUZ, UNMUZ = G.COM_MOVE, G.COM_WAKE, G.COM_MUZZLE, G.COM_UNMUZZLE
NAMES = ("MOVED", "MOVED_UNSEEN", "MUZZLED", "UNMUZZLED", "WOKEN", "MOVE_USAGE", "MOVE_NOBODY", "MOVE_NO_ROOM", "MOVE_SELF", "MOVE_LEVEL",
         "MOVE_ALREADY", "MOVE_PRIVATE", "MOVE_AWAY", "WAKE_USAGE", "WAKE_MUZZLED", "WAKE_NOBODY", "WAKE_SELF", "WAKE_AFK", "MUZZLE_USAGE",
         "MUZZLE_ABSENT", "MUZZLE_SELF", "MUZZLE_LEVEL", "MUZZLE_ALREADY", "UNMUZZLE_USAGE", "UNMUZZLE_ABSENT", "UNMUZZLE_SELF",
         "UNMUZZLE_NOT", "UNMUZZLE_ABOVE", "DEFERRED")
MAXES = ("MAX_ACT_HERE", "MAX_ACT_ENTER", "MAX_ACT_LEAVE", "MAX_ACT_RESET", "MAX_ACT_REPLY", "MAX_ACT_NOTICE")


def hand_rooms() -> list:
    """drive (fixed public) - hallway - den (private) - attic; the hallway also adjoins the vault (fixed private)."""
    return [list_room(b"drive", links=[1], access=G.FIXED_PUBLIC), list_room(b"hallway", links=[0, 2, 4]),
            list_room(b"den", links=[1, 3], access=G.PRIVATE), list_room(b"attic", links=[2]),
            list_room(b"vault", links=[1], access=G.FIXED_PRIVATE)]


def hand_users() -> dict:
    """Alice and the invisible ARCH Dave in the hallway, Bobby and the WIZ Carol in the private den, Erica in the attic, the
    GOD Gina in the drive; a nameless slot, a login slot, a slot without a room, and Remo in a room without a record."""
    return {0: act_user(0, name=b"Alice", room=1, colour=1), 1: act_user(1, name=b"Bobby", room=2), 2: act_user(2, name=b"Carol", room=2, level=WIZ),
            3: act_user(3, name=b"Dave", room=1, level=ARCH, vis=0), 4: act_user(4, name=b"Erica", room=3, invite=2, ignall=1),
            5: act_user(5, name=None, room=1), 6: act_user(6, name=b"Prompt", room=1, login=1), 7: act_user(7, name=None, room=None),
            8: act_user(8, name=b"Gina", room=0, level=GOD), 9: act_user(9, name=b"Remo", room=77)}


def seated(capacity=10, **kw):
    rms, users = hand_rooms(), hand_users()
    r = device.Roster(capacity, look_rooms=len(rms), **kw)
    set_rooms(r, rms)
    seat_all(r, users)
    return r, users, rms


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


# ------------------------------------------------------------------ host tier: names and input checks
def test_the_new_names_exist():
    assert (G.COM_MOVE, G.COM_WAKE, G.COM_MUZZLE, G.COM_UNMUZZLE) == (21, 58, 60, 61)
    assert [nuts_path.lib().np_command_name(c) for c in (21, 58, 60, 61)] == [b"move", b"wake", b"muzzle", b"unmuzzle"]
    assert G.ACT_KERNELS == ("nuts_roster_act", "nuts_roster_act_order")
    assert not set(G.ACT_KERNELS) & (set(G.KERNELS) | set(G.GO_KERNELS) | set(G.ACCESS_KERNELS) | set(G.CLONE_KERNELS) | set(G.SET_KERNELS))
    source = device.SOURCE.read_text()
    assert "nuts_roster_act(ActArgs a)" in source and "nuts_roster_act_order(ActOrderArgs a)" in source
    assert [getattr(G, "ACT_" + n) for n in NAMES] == list(range(29))
    for n in NAMES:                                                     # the kernel's constants, by the same names and numbers
        assert f"kAct{n.title().replace('_', '')} = {getattr(G, 'ACT_' + n)}" in source, n
    assert tuple(getattr(G, m) for m in MAXES) == (46, 55, 80, 35, 84, 72)
    assert G._ACT_ROWS == (48, 56, 80, 36, 84, 72) and all(m <= row < m + 4 and row % 4 == 0 for m, row in zip(
        (getattr(G, m) for m in MAXES), G._ACT_ROWS))
    assert ("constexpr int kActHereRow = 48, kActEnterRow = 56, kActLeaveRow = 80, kActResetRow = 36, kActReplyRow = 84, "
            "kActNoticeRow = 72;") in source
    assert ("kActHereMax == 46 && kActEnterMax == 55 && kActLeaveMax == 80 && kActResetMax == 35 && kActReplyMax == 84 && "
            "kActNoticeMax == 72") in source
    assert (G.ACT_HERE, G.ACT_ENTER, G.ACT_LEAVE, G.ACT_RESET, G.ACT_REPLY, G.ACT_NOTICE) == (0, 1, 2, 3, 4, 5)
    assert f"kMuzzleByte = kNameLen + 3" in source and G._MUZZLE_BYTE == G.USER_NAME_LEN + 3 == 15 and G.LEVEL_WIZ == WIZ
    assert callable(G.Roster.act_many) and G.Act.__dataclass_fields__.keys() >= {
        "outcome", "target_slot", "target_room", "old_room", "returned_public", "reply", "here", "enter", "leave", "reset", "notice",
        "texts", "text_starts", "text_sizes", "look", "look_index", "timing"}
    # the shared loops: each written once; the new kernel's argument has a name of its own
    assert source.count("wave_get_room(e.rooms") == 1 and source.count("wave_get_user(e.speech") == 1
    doc = G.Roster.act_many.__doc__
    assert all(word in doc for word in ("reply, the here line, the notice, the enter", "ACT_MOVE_AWAY", "``*_ABSENT``", "syslog", "``prompt(u)``",
                                        "relay_many", "remote users", "input_many", "ACT_DEFERRED", "at most twice"))
    assert "act_many" in G.Roster.go_many.__doc__ and "``.move``" in G.Roster.go_many.__doc__
    assert "act_many" in G.Roster.access_many.__doc__ and "``.move``" in G.Roster.access_many.__doc__
    assert "act_many" in device.__doc__ and "muzzle_level" in G.Roster.update.__doc__


@pytest.mark.parametrize("events, why", [
    ([], "empty call"), ((), "empty call"), (None, "events must be a sequence"), ("x", "events must be a sequence"),
    ([(0, b"bobby", 2)], "event 0: expected a \\(slot, com, inpstr, word_count\\) tuple"), ([[0, MOVE, b"bobby", 2]], "event 0: expected"),
    ([(0, WAKE, b"", 1), (10, WAKE, b"", 1)], "event 1: slot"), ([(True, WAKE, b"", 1)], "event 0: slot"),
    ([(0, 20, b"", 1)], "event 0: com must be"), ([(0, 59, b"", 1)], "event 0: com must be"), ([(0, G.COM_GO, b"den", 2)], "event 0: com must be"),
    ([(0, 62, b"", 1)], "event 0: com must be"), ([(0, True, b"", 1)], "event 0: com must be"), ([(0, None, b"", 1)], "event 0: com must be"),
    ([(0, MOVE, 5, 2)], "event 0: inpstr|event 0: text"), ([(0, MUZ, b"a\0b", 2)], "event 0: text contains a NUL"),
    ([(0, UNMUZ, b"x" * 1000, 2)], "event 0: inpstr of 1000 bytes"), ([(0, MOVE, b"bobby", 11)], "event 0: word_count"),
    ([(0, WAKE, b"bobby", -1)], "event 0: word_count"), ([(0, MUZ, b"bobby", None)], "event 0: word_count"),
    ([(0, WAKE, b"", 1), (5, WAKE, b"", 1)], "event 1: the actor, slot 5, has no name"),
    ([(6, MOVE, b"", 1)], "event 0: the actor, slot 6, is still logging in"), ([(7, MUZ, b"", 1)], "event 0: the actor, slot 7, is in no room"),
    ([(9, UNMUZ, b"", 1)], "event 0: the actor, slot 9, is in room 77, which has no room record"),
])
def test_malformed_events_are_rejected_before_the_library_loads(no_library, events, why):
    r, _, _ = seated()
    clean(r)
    before = mirrors(r)
    with pytest.raises(ValueError, match=why):
        r.act_many(events, **KW)
    assert flags(r) == (False,) * len(FLAGS) and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))


@pytest.mark.parametrize("kw, why", [
    ({"gatecrash_level": 5}, "gatecrash_level"), ({"gatecrash_level": -1}, "gatecrash_level"), ({"gatecrash_level": True}, "gatecrash_level"),
    ({"min_private_users": -1}, "min_private_users"), ({"min_private_users": 2.0}, "min_private_users"),
    ({"min_private_users": 2**31}, "min_private_users"), ({"min_private_users": None}, "min_private_users"),
])
def test_the_two_settings_are_checked(no_library, kw, why):
    r, _, _ = seated()
    clean(r)
    before = mirrors(r)
    with pytest.raises(ValueError, match=why):
        r.act_many([(0, WAKE, b"", 1)], **{**KW, **kw})
    assert flags(r) == (False,) * len(FLAGS) and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))
    for missing in KW:
        with pytest.raises(TypeError):
            r.act_many([(0, WAKE, b"", 1)], **{k: v for k, v in KW.items() if k != missing})
    with pytest.raises(TypeError):
        r.act_many([(0, WAKE, b"", 1)], 3, 2)                           # keyword-only


def test_a_roster_without_rooms_a_closed_one_and_a_call_past_the_cap(no_library, monkeypatch):
    r = device.Roster(4)
    r.update(0, room=0, name=b"Alice")
    with pytest.raises(ValueError, match=r"no room records \(look_rooms is 0\)"):
        r.act_many([(0, WAKE, b"", 1)], **KW)
    r, _, _ = seated()
    state, before = flags(r), mirrors(r)
    bound = 12 * sum(G._ACT_ROWS) * 2 + 16 * 12
    monkeypatch.setattr(device, "MANY_ARENA_CAP", bound - 1)
    with pytest.raises(ValueError, match=f"call too large: its variant bound is {bound} bytes.*MANY_ARENA_CAP.*split it"):
        r.act_many([(0, WAKE, b"", 1), (0, MUZ, b"", 1)], **KW)
    assert flags(r) == state and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))
    r.close()
    with pytest.raises(ValueError, match="closed"):
        r.act_many([(0, WAKE, b"", 1)], **KW)


# ------------------------------------------------------------------ host tier: update(muzzle_level=)
def test_update_muzzle_level_sets_byte_15_the_bit_and_the_dirty_flag():
    r = device.Roster(4)
    r.update([0, 1, 2], name=[b"Ann", b"Ben", b"Cy"], room=0, level=[1, 2, 3])
    clean(r)
    before = r._speech.copy()
    r.update([0, 1], muzzle_level=[ARCH, 0])
    assert flags(r) == only("_speech_dirty")                            # as level= marks it, and nothing else
    assert r._speech[0, 15] == ARCH and r._speech[0, 13] & G.SPEECH_FLAGS["muzzled"] and r._speech[1, 15] == 0
    assert not r._speech[1, 13] & G.SPEECH_FLAGS["muzzled"]
    assert np.array_equal(r._speech[:, :13], before[:, :13]) and np.array_equal(r._speech[:, 14], before[:, 14]) and np.array_equal(r._speech[2:], before[2:])
    r.update(0, muzzle_level=0)                                         # removed: the bit goes with it
    assert r._speech[0, 15] == 0 and not r._speech[0, 13] & G.SPEECH_FLAGS["muzzled"]
    # muzzled= alone writes the bit and leaves byte 15 as it was
    r.update(2, muzzle_level=GOD)
    r.update(2, muzzled=0)
    assert r._speech[2, 15] == GOD and not r._speech[2, 13] & G.SPEECH_FLAGS["muzzled"]
    r.update(1, muzzled=1)
    assert r._speech[1, 15] == 0 and r._speech[1, 13] & G.SPEECH_FLAGS["muzzled"]
    state, kept = flags(r), r._speech.copy()
    for bad, why in (({"muzzle_level": 5}, "muzzle_level must be an int"), ({"muzzle_level": -1}, "muzzle_level"), ({"muzzle_level": True}, "muzzle_level"),
                     ({"muzzle_level": None}, "muzzle_level"), ({"muzzle_level": [1, 2]}, "muzzle_level: 2 values for 1 slots"),
                     ({"muzzle_level": 2, "muzzled": 1}, "cannot be given in one update"), ({"muzzle_level": 0, "muzzled": 0}, "cannot be given")):
        with pytest.raises(ValueError, match=why):
            r.update(0, **bad)
    assert flags(r) == state and np.array_equal(r._speech, kept)
    assert "byte 15" in G.Roster.update.__doc__ and "WIZ" in G.Roster.update.__doc__


def test_how_a_muzzle_is_read():
    assert [muzzle_of({"muzzled": b, "muzzle": m}) for b, m in ((0, 0), (0, GOD), (1, 0), (1, ARCH), (1, GOD))] == [0, 0, WIZ, ARCH, GOD]
    source = device.SOURCE.read_text()
    assert "!(tp[kNameLen + 1] & kMuzzled) ? 0 : tp[kMuzzleByte] ? tp[kMuzzleByte] : kWiz" in source


# ------------------------------------------------------------------ host tier: the model against the recordings
#: the outcomes act.json does not reach: the netlink release, as the generator's docstring says, and what one event never is
EXCUSED = {G.ACT_MOVE_AWAY, G.ACT_DEFERRED}


@pytest.fixture(scope="module")
def model_replays():
    return {name: (load(name), ActReplayer(load(name)).run()) for name in SESSIONS}


def test_the_model_reproduces_every_step_of_the_recorded_sessions(model_replays):
    for name, (doc, res) in model_replays.items():
        assert res["mismatches"] == [], (name, res["mismatches"][:1])
        assert res["act"] == res["act_lines"] == act_lines(doc), name                  # none is left out
        assert res["answered"] + res["state_only"] == sum(s["op"] == "line" for s in doc["steps"])
        assert res["plan_disagreements"] == 0 and res["comparisons"] > 0
    # the new session; the clone session's .muzzle and .unmuzzle, whose .csay reads the muzzle act_many set; a seeded one
    assert [res["act"] for _, res in model_replays.values()] == [37, 2, 0]
    assert [res["state_only"] for _, res in model_replays.values()] == [2, 0, 0]        # the .afk and the return from it


def test_what_the_new_recording_holds(model_replays):
    doc, res = model_replays["reference_only/act.json"]
    assert doc["config"] == {"max_clones": 1, "min_private": 2, "ignore_mp_level": WIZ, "gatecrash_level": ARCH}
    assert [(a["level"], a["colour"]) for a in doc["accounts"][0]] == [(1, 1), (1, 0), (2, 0), (3, 1), (4, 0)]
    assert set(res["act_outcomes"]) == set(range(29)) - EXCUSED, res["act_outcomes"]
    assert "ACT_MOVE_AWAY" in (sr.REPO / "tests" / "golden" / "make_act_golden.py").read_text()
    assert 50 <= sum(1 for s in doc["steps"] if s["op"] == "line") <= 110
    by_note = {s["note"]: s for s in doc["steps"] if s.get("note")}
    mine = lambda note: by_note[note]["recv"][by_note[note]["actor"]]
    out = by_note["out of the actor's room"]["recv"]                     # the target hears the chant line, then the giant hand
    assert out["c"].index("Dave chants an ancient spell...") < out["c"].index("A giant hand grabs you")
    assert "A giant hand grabs Carol who is pulled into a magical blue vortex!" in out["a"]
    own = mine("into the actor's own room")                             # the actor hears the enter line after its reply
    assert own.index("You chant an ancient spell...") < own.index("Carol falls out of a magical blue vortex!")
    assert mine("move refused as private") == "The corridor is currently private, Alice cannot be moved there.\n\r"
    assert "Room access returned to" in by_note["the room returns to public"]["recv"]["a"] and "Review buffer is empty." in mine("the buffer is empty")
    assert mine("the invitation is gone") == "That room is currently private, you cannot enter.\n\r"
    assert "A presence chants an ancient spell..." in by_note["an invisible actor"]["recv"]["c"]
    unseen = by_note["an invisible target"]["recv"]
    assert unseen["b"] == "A presence leaves the room.\n\r" and "giant hand" not in unseen["d"] and "Gina chants" in unseen["a"]
    assert "[ hallway ]:" in by_note["past a clone that relays"]["recv"]["d"] and by_note["an ignall listener"]["recv"].get("b", "") == ""
    assert by_note["woken"]["recv"]["b"] == "\x07\n\r*** Alice says: WAKE UP!!! ***\n\r\n\r"
    assert "A presence says: " in by_note["woken by an invisible actor"]["recv"]["a"]
    assert by_note["a user goes AFK"]["send"] == ".afk" and by_note["wake AFK"]["recv"].get("b", "") == ""
    assert mine("wake AFK") == "You cannot wake someone who is AFK.\x1b[0m\n\r\x1b[0m" and "no longer AFK" in mine("the return from AFK")
    assert mine("muzzled by the WIZ") == "Alice now has a muzzle of level: WIZ.\n\r" and "ARCH." in mine("muzzled by the ARCH")
    assert mine("unmuzzle above the level") == "Alice's muzzle is set to level ARCH, you do not have the power to remove it.\n\r"
    assert mine("a muzzled say") == "You are muzzled, you cannot speak.\x1b[0m\n\r\x1b[0m" or "You are muzzled, you cannot speak." in mine("a muzzled say")
    assert "You are muzzled, you cannot wake anyone." in mine("a muzzled wake")
    assert by_note["not muzzled: nothing is written"]["recv"].get("c", "") == ""        # the reference sprintf()s and writes nothing
    assert mine("muzzle absent") == mine("unmuzzle absent") == "There is no such user.\n\r"


# ------------------------------------------------------------------ host tier: the decision chain
def one(users, rms, slot, com, line=b"", wc=None, gate=ARCH, minp=2, clones=()):
    return act(users, rms, list(clones), slot, com, line, len(line.split()) + 1 if wc is None else wc, gate, minp)


def test_the_decision_chain_of_move():
    users, rms = hand_users(), hand_rooms()
    go = lambda slot, line=b"", **kw: one(users, rms, slot, MOVE, line, **kw)
    assert go(8)["reply"] == b"Usage: move <user> [<room>]\n" and go(8)["outcome"] == G.ACT_MOVE_USAGE
    assert go(8, b"zed attic")["outcome"] == G.ACT_MOVE_NOBODY and go(8, b"zed nosuch")["target_room"] == -1      # get_room is not reached
    assert go(8, b"prompt")["outcome"] == G.ACT_MOVE_NOBODY and go(8, b"zed")["reply"] == b"There is no one of that name logged on.\n"
    assert go(8, b"alice nosuch")["reply"] == b"There is no such room.\n" and go(8, b"alice nosuch")["target_slot"] == 0
    assert go(8, b"gin attic")["outcome"] == G.ACT_MOVE_SELF and go(8, b"gin nosuch")["outcome"] == G.ACT_MOVE_NO_ROOM  # the room comes first
    assert go(2, b"dave")["outcome"] == G.ACT_MOVE_LEVEL and go(2, b"carol")["outcome"] == G.ACT_MOVE_SELF
    assert go(2, b"bob")["reply"] == b"Bobby is already in the den.\n" and go(8, b"alice hall")["outcome"] == G.ACT_MOVE_ALREADY
    assert go(8, b"alice hall", wc=2)["outcome"] == G.ACT_MOVED                         # word_count decides, not the words: into the drive
    # has_room_access is the ACTOR's: Carol, a WIZ below the gatecrash level, may not move Alice into the private den from
    # elsewhere, but into the fixed-private vault, and where she is invited; the target's own invitation does not count
    users[2]["room"] = 3
    assert go(2, b"alice den")["reply"] == b"The den is currently private, Alice cannot be moved there.\n"
    assert go(2, b"alice vault")["outcome"] == G.ACT_MOVED and go(2, b"erica den")["outcome"] == G.ACT_MOVE_PRIVATE
    users[2]["invite"] = 2
    assert go(2, b"alice den")["outcome"] == G.ACT_MOVED and go(2, b"alice den", gate=WIZ)["outcome"] == G.ACT_MOVED
    users[2].update(invite=None, room=2)
    assert go(8, b"remo")["outcome"] == G.ACT_MOVE_AWAY and go(8, b"remo")["reply"] is None     # the caller's branch
    users[9]["room"] = None
    assert go(8, b"remo attic")["outcome"] == G.ACT_MOVE_AWAY and go(8, b"remo attic")["old"] == -1
    got = go(8, b"bob attic")
    assert (got["outcome"], got["target_slot"], got["target_room"], got["old"], got["returned"]) == (G.ACT_MOVED, 1, 3, 2, True)
    assert got["reply"] == b"~FT~OLYou chant an ancient spell...\n" and got["here"] == b"~FT~OLGina chants an ancient spell...\n"
    assert got["notice"] == b"\n~FT~OLA giant hand grabs you and pulls you into a magical blue vortex!\n"
    assert got["enter"] == b"~FT~OLBobby falls out of a magical blue vortex!\n" and got["reset"] == b"Room access returned to ~FGPUBLIC.\n"
    assert got["leave"] == b"~FT~OLA giant hand grabs Bobby who is pulled into a magical blue vortex!\n"
    assert go(8, b"bob attic", minp=1)["returned"] is False and go(8, b"bob attic", clones=[(0, 2, 2)])["returned"] is False
    unseen = go(8, b"dave")                                             # an invisible target: no giant hand for it
    assert (unseen["outcome"], unseen["notice"], unseen["enter"], unseen["leave"]) == (
        G.ACT_MOVED_UNSEEN, None, b"A presence enters the room...\n", b"A presence leaves the room.\n")
    users[8]["vis"] = 0
    assert go(8, b"alice")["here"] == b"~FT~OLA presence chants an ancient spell...\n"


def test_the_decision_chains_of_wake_muzzle_and_unmuzzle():
    users, rms = hand_users(), hand_rooms()
    wake = lambda slot, line=b"", **kw: one(users, rms, slot, WAKE, line, **kw)
    assert wake(0)["reply"] == b"Usage: wake <user>\n" and wake(0, b"zed")["outcome"] == G.ACT_WAKE_NOBODY
    assert wake(0, b"ali")["reply"] == b"Trying to wake yourself up is the eighth sign of madness.\n"
    users[1]["afk"] = 1
    assert wake(0, b"bobby")["reply"] == b"You cannot wake someone who is AFK.\n"
    got = wake(0, b"carol")
    assert (got["outcome"], got["reply"], got["target_slot"]) == (G.ACT_WOKEN, b"Wake up call sent.\n", 2)
    assert got["notice"] == b"\07\n~BR*** Alice says: ~OL~LIWAKE UP!!!~RS~BR ***\n\n" and got["target_room"] == 1 and got["old"] == 2
    assert wake(3, b"carol")["notice"] == b"\07\n~BR*** A presence says: ~OL~LIWAKE UP!!!~RS~BR ***\n\n"
    users[0]["muzzled"] = 1                                             # the bit alone refuses: before get_user, after the usage
    assert wake(0, b"zed")["reply"] == b"You are muzzled, you cannot wake anyone.\n" and wake(0)["outcome"] == G.ACT_WAKE_USAGE
    muz = lambda slot, line=b"", **kw: one(users, rms, slot, MUZ, line, **kw)
    assert muz(2)["reply"] == b"Usage: muzzle <user>\n" and muz(2, b"zed")["outcome"] == G.ACT_MUZZLE_ABSENT and muz(2, b"zed")["reply"] is None
    assert muz(2, b"car")["reply"] == b"Trying to muzzle yourself is the ninth sign of madness.\n"
    assert muz(2, b"dave")["reply"] == b"You cannot muzzle a user of equal or higher level than yourself.\n"
    assert muz(2, b"alice")["reply"] == b"Alice is already muzzled.\n"                  # the bit over byte 0 reads as WIZ: >= Carol's level
    got = muz(3, b"alice")                                              # below the ARCH's
    assert (got["outcome"], got["notice"]) == (G.ACT_MUZZLED, b"~FR~OLYou have been muzzled!\n")
    assert got["reply"] == b"~FR~OLAlice now has a muzzle of level: ~RS~OLARCH.\n"
    unm = lambda slot, line=b"", **kw: one(users, rms, slot, UNMUZ, line, **kw)
    assert unm(2)["reply"] == b"Usage: unmuzzle <user>\n" and unm(2, b"zed")["outcome"] == G.ACT_UNMUZZLE_ABSENT
    assert unm(2, b"car")["reply"] == b"Trying to unmuzzle yourself is the tenth sign of madness.\n"
    silent = unm(2, b"bobby")                                           # the reference sprintf()s and writes nothing
    assert silent["outcome"] == G.ACT_UNMUZZLE_NOT and all(silent[kind] is None for kind in KINDS)
    users[1].update(muzzled=1, muzzle=GOD)
    assert unm(2, b"bobby")["reply"] == b"Bobby's muzzle is set to level GOD, you do not have the power to remove it.\n"
    users[1]["muzzle"] = WIZ
    got = unm(2, b"bobby")                                              # not above: a WIZ removes a WIZ's muzzle, even from an equal
    assert (got["outcome"], got["reply"], got["notice"]) == (G.ACT_UNMUZZLED, b"~FG~OLYou remove Bobby's muzzle.\n", b"~FG~OLYou have been unmuzzled!\n")


# ------------------------------------------------------------------ host tier: the deferral rule
def outcomes(call):
    return [e["outcome"] for e in call["events"]]


def call_of(users, rms, events, clones=(), gate=ARCH, minp=2):
    return act_call(users, rms, list(clones), events, gate, minp)


def test_one_event_never_defers_and_refusals_touch_nothing():
    users, rms = hand_users(), hand_rooms()
    for ev in ((8, MOVE, b"bobby attic", 3), (3, MUZ, b"alice", 2), (0, WAKE, b"carol", 2), (2, UNMUZ, b"bobby", 2)):
        assert outcomes(call_of(hand_users(), hand_rooms(), [ev]))[0] != G.ACT_DEFERRED
    events = [(0, WAKE, b"carol", 2), (0, WAKE, b"carol", 2), (2, MUZ, b"dave", 2), (2, MOVE, b"dave", 2), (2, UNMUZ, b"alice", 2), (8, MOVE, b"remo", 2)]
    call = call_of(users, rms, events)
    assert outcomes(call) == [G.ACT_WOKEN, G.ACT_WOKEN, G.ACT_MUZZLE_LEVEL, G.ACT_MOVE_LEVEL, G.ACT_UNMUZZLE_NOT, G.ACT_MOVE_AWAY]
    assert call["events"][0]["plans"]["notice"] == [2] and call["events"][0]["plans"]["reply"] == [0]


def test_the_deferral_rule_key_by_key():
    # Gina moves Bobby from the den to the attic: Bobby's slot, the den and the attic are touched
    first = (8, MOVE, b"bobby attic", 3)
    for second, why in (((1, WAKE, b"alice", 2), "the actor's slot"), ((0, WAKE, b"bobby", 2), "the found slot"),
                        ((2, WAKE, b"alice", 2), "the actor's room: the den was left"), ((0, WAKE, b"carol", 2), "the found slot's room"),
                        ((3, MOVE, b"alice attic", 3), "the resolved room: the attic was entered"),
                        ((4, WAKE, b"alice", 2), "the actor's room: the attic was entered")):
        call = call_of(hand_users(), hand_rooms(), [first, second])
        assert outcomes(call) == [G.ACT_MOVED, G.ACT_DEFERRED], why
        assert all(call["events"][1][kind] is None and call["events"][1]["plans"][kind] == [] for kind in KINDS), why
    # what shares none of the five is answered; a deferred event touches nothing itself
    users, rms = hand_users(), hand_rooms()
    call = call_of(users, rms, [first, (0, WAKE, b"dave", 2), (3, MOVE, b"alice attic", 3), (3, MUZ, b"alice", 2), (0, WAKE, b"dave", 2)])
    assert outcomes(call) == [G.ACT_MOVED, G.ACT_WOKEN, G.ACT_DEFERRED, G.ACT_MUZZLED, G.ACT_DEFERRED]
    assert users[1]["room"] == 3 and users[0]["room"] == 1 and users[0]["muzzled"] == 1 and users[0]["muzzle"] == ARCH
    assert rms[2]["access"] == G.PUBLIC and call["cleared"] == [2] and users[4]["invite"] is None and call["movers"] == [1]
    # a muzzle touches the target's slot alone: its room-mates are answered, the muzzled one's own wake waits
    call = call_of(hand_users(), hand_rooms(), [(3, MUZ, b"alice", 2), (3, WAKE, b"carol", 2), (0, WAKE, b"carol", 2), (8, UNMUZ, b"alice", 2)])
    assert outcomes(call) == [G.ACT_MUZZLED, G.ACT_WOKEN, G.ACT_DEFERRED, G.ACT_DEFERRED]
    # submitted again the wake is refused: decided against the snapshot it would have been sent
    users, rms = hand_users(), hand_rooms()
    call_of(users, rms, [(3, MUZ, b"alice", 2)])
    assert outcomes(call_of(users, rms, [(0, WAKE, b"carol", 2)])) == [G.ACT_WAKE_MUZZLED]
    # the binding's own: the den returns to public, and a move into the hallway, which adjoins it, waits for the next call
    call = call_of(hand_users(), hand_rooms(), [(8, MOVE, b"bobby attic", 3), (8, MOVE, b"remo", 2), (3, MOVE, b"gina hall", 3)])
    assert outcomes(call) == [G.ACT_MOVED, G.ACT_MOVE_AWAY, G.ACT_MOVE_LEVEL]
    users = hand_users()
    users[8]["level"] = WIZ
    assert outcomes(call_of(users, hand_rooms(), [(3, MOVE, b"bobby attic", 3), (3, MOVE, b"gina hall", 3)])) == [G.ACT_MOVED, G.ACT_DEFERRED]


def test_the_seeded_stream_of_the_model_holds_every_outcome():
    f = fuzz_part(20263, on_device=False)                               # the child's default seed
    assert set(f["outcomes"]) == {str(o) for o in range(29)}, f["outcomes"]


# ------------------------------------------------------------------ host tier: the bounds
def test_the_longest_texts_stay_within_their_rows():
    users = {0: act_user(0, name=b"N" * 12, room=0, level=GOD), 1: act_user(1, name=b"W" * 12, room=1, muzzled=1, muzzle=GOD),
             2: act_user(2, name=b"I" * 12, room=0, vis=0, level=ARCH), 3: act_user(3, name=b"T" * 12, room=2, muzzled=1, muzzle=ARCH),
             4: act_user(4, name=b"Z" * 12, room=0, level=WIZ)}
    rms = [list_room(b"r" * 20, links=[1]), list_room(b"p" * 20, links=[0], access=G.PRIVATE), list_room(b"t" * 20, access=G.FIXED_PRIVATE)]
    events = [(0, MOVE, b"W" * 12 + b" t", 3), (0, MOVE, b"I" * 12 + b" p", 3), (2, MOVE, b"T" * 12 + b" " + b"p" * 20, 3),
              (0, MOVE, b"T" * 12 + b" t", 3), (2, WAKE, b"T" * 12, 2), (0, WAKE, b"T" * 12, 2), (2, MUZ, b"W" * 12, 2), (0, MUZ, b"I" * 12, 2),
              (2, UNMUZ, b"W" * 12, 2), (0, UNMUZ, b"T" * 12, 2), (0, MOVE, b"N" * 12, 2), (2, MUZ, b"N" * 12, 2), (0, MUZ, b"T" * 12, 2),
              (4, UNMUZ, b"T" * 12, 2), (0, MUZ, b"W" * 12, 2)]
    results = [act(users, rms, [], s, c, w, wc, GOD, 2**31 - 1) for s, c, w, wc in events]
    longest = dict.fromkeys(KINDS, 0)
    for res in results:
        for kind, most, row in zip(KINDS, (G.MAX_ACT_HERE, G.MAX_ACT_ENTER, G.MAX_ACT_LEAVE, G.MAX_ACT_RESET, G.MAX_ACT_REPLY, G.MAX_ACT_NOTICE), G._ACT_ROWS):
            text = res[kind]
            if text is None:
                continue
            longest[kind] = max(longest[kind], len(text))
            assert len(text) <= most <= row
            for c in (0, 1):
                ch = nuts_path.chunks(text, c)
                assert sum(map(len, ch)) <= device.max_bytes(most) and len(ch) <= device.MAX_WRITES
    assert longest == {"here": 46, "enter": 55, "leave": 80, "reset": 35, "reply": 84, "notice": 72}
    assert results[2]["reply"] == b"The " + b"p" * 20 + b" is currently private, " + b"T" * 12 + b" cannot be moved there.\n"
    assert {r["outcome"] for r in results} >= {G.ACT_MOVED, G.ACT_MOVED_UNSEEN, G.ACT_MOVE_PRIVATE, G.ACT_MOVE_ALREADY, G.ACT_WOKEN, G.ACT_MUZZLED,
                                               G.ACT_UNMUZZLE_ABOVE, G.ACT_UNMUZZLED, G.ACT_MOVE_SELF, G.ACT_MUZZLE_LEVEL, G.ACT_MUZZLE_ALREADY}


# ------------------------------------------------------------------ the apply step, over a library that computes nothing
ACT_MIRROR_ARGS = {11: "_table", 12: "_speech", 13: "_clones", 14: "_rooms", 15: "_go"}


class ActFakeLibrary(FakeLibrary):
    """The go tests' library that computes nothing; ``nd_roster_act`` answers with the next entry of ``act_script``: per
    event ``(outcome, target_slot, target_room, old_room, returned)``."""

    def __init__(self, arrays: dict):
        super().__init__(arrays)
        self.act_script = []

    def __getattr__(self, name):
        call = super().__getattr__(name)
        if name != "nd_roster_act":
            return call

        def act_(*args):
            call(*args)
            answer = self.act_script.pop(0)
            for col, at in enumerate((16, 17, 18, 19, 20)):
                self.arrays[args[at]][:] = [e[col] for e in answer]
            self.arrays[args[21]][:] = -1
            for at in (23, 24):
                self.arrays[args[at]][:] = 0
            return 0
        return act_


@pytest.fixture
def fake(monkeypatch):
    arrays: dict = {}
    lib = ActFakeLibrary(arrays)
    real = device._ptr

    def ptr(a):
        arrays[a.ctypes.data] = a
        return real(a)

    monkeypatch.setattr(device, "_ptr", ptr)
    monkeypatch.setattr(device, "_load", lambda: lib)
    return lib


def scripted(lib, users, rms, clones, events, gate=ARCH, minp=2):
    call = act_call(users, rms, clones, events, gate, minp)
    lib.act_script.append([(e["outcome"], e["target_slot"], e["target_room"], e["old"], int(e["returned"])) for e in call["events"]])
    return call


def muzzles_differ(r, users) -> list:
    return [j for j, u in users.items() if (int(r._speech[j, 13] >> 1 & 1), int(r._speech[j, 15])) != (int(bool(u["muzzled"])), u["muzzle"])]


QUIET = ("_afk_dirty", "_udesc_dirty", "_who_dirty")


def test_act_many_is_passed_exactly_the_dirty_mirrors_and_applies_the_result(fake):
    r, users, rms = seated(10, clones=2, review_rooms=3)
    clones = [(0, 2, device.CLONE_HEAR_ALL), None]
    seat_clones(r, clones)
    scripted(fake, users, rms, clones, [(0, WAKE, b"", 1)])
    got = r.act_many([(0, WAKE, b"", 1)], **KW)
    name, args = fake.calls[-1]
    assert name == "nd_roster_act" and args[1] == 1 and args[9:11] == (ARCH, 2) and len(args) == 29
    assert all(args[i] == getattr(r, m).ctypes.data for i, m in ACT_MIRROR_ARGS.items())
    assert flags(r) == only(*QUIET) and got.effective().tolist() == [] and got.moved().tolist() == [] and len(fake.calls) == 1
    scripted(fake, users, rms, clones, [(0, WAKE, b"x", 2)])
    r.act_many([(0, WAKE, b"x", 2)], **KW)
    assert passed(fake, r) == set()                                     # nothing changed: nothing travels
    for fields, want in (({"invite_room": 1}, {"_go"}), ({"room": 1}, {"_table"}), ({"level": 1}, {"_speech"}), ({"muzzle_level": 0}, {"_speech"}),
                         ({"afk": 1}, {"_speech"}), ({"igntell": 1}, {"_speech"}),  # a .wake reads afk: the flags byte travels
                         ({"desc": b"d"}, set()), ({"afk_mesg": b"brb"}, set()), ({"last_login": 4}, set())):
        r.update(0, **fields)
        users[0].update({("invite" if f == "invite_room" else f): v for f, v in fields.items() if f in ("invite_room", "level")})
        scripted(fake, users, rms, clones, [(0, WAKE, b"x", 2)])
        r.act_many([(0, WAKE, b"x", 2)], **KW)
        assert passed(fake, r) == want, fields
    r.set_rooms(3, topic=b"t")
    r.set_clones(1, owner=1, room=1)
    clones[1] = (1, 1, device.CLONE_HEAR_ALL)
    scripted(fake, users, rms, clones, [(0, WAKE, b"x", 2)])
    r.act_many([(0, WAKE, b"x", 2)], **KW)
    assert passed(fake, r) == {"_rooms", "_clones"} and not r._rooms_dirty and not r._clones_dirty
    # a muzzle: the speaker table alone is stale afterwards, and a following speak_many is passed it again
    call = scripted(fake, users, rms, clones, [(3, MUZ, b"alice", 2)])
    got = r.act_many([(3, MUZ, b"alice", 2)], **KW)
    assert outcomes(call) == [G.ACT_MUZZLED] and got.effective().tolist() == [0] and got.look is None and len(fake.calls[-1][1]) == 29
    assert flags(r) == only(*QUIET, "_speech_dirty") and r._speech[0, 15] == ARCH and r._speech[0, 13] & 2
    assert muzzles_differ(r, users) == [] and model_state_differences(r, users, rms) == []
    r.speak_many([(0, G.COM_SAY, b"hello", 2)])
    assert fake.calls[-1][0] == "nd_roster_speak" and "_speech" in passed(fake, r) and not r._speech_dirty
    scripted(fake, users, rms, clones, [(8, UNMUZ, b"alice", 2)])
    r.act_many([(8, UNMUZ, b"alice", 2)], **KW)
    assert muzzles_differ(r, users) == [] and r._speech[0, 15] == 0 and not r._speech[0, 13] & 2 and r._speech_dirty
    # a move out of the private den, which returns to public: the second visit is the look, which is passed the table
    r.plan_many([(b"in the den's ring\n", 2, None, 0, device.COM_SAY)], record=True)
    before = len(fake.calls)
    call = scripted(fake, users, rms, clones, [(8, MOVE, b"carol attic", 3), (0, WAKE, b"carol", 2)])
    got = r.act_many([(8, MOVE, b"carol attic", 3), (0, WAKE, b"carol", 2)], **KW)
    assert outcomes(call) == got.outcome.tolist() == [G.ACT_MOVED, G.ACT_DEFERRED] and got.returned_public.tolist() == [False, False]
    assert [c[0] for c in fake.calls[before:]] == ["nd_roster_act", "nd_roster_look"]  # at most two device visits
    assert "_table" in passed(fake, r) and got.look.slots.tolist() == [2] and got.look_index.tolist() == [0, -1]
    assert model_state_differences(r, users, rms) == [] and int(r._room[2]) == 3
    users[4]["invite"] = 2                                              # Erica is invited into the den again
    r.update(4, invite_room=2)
    before = len(fake.calls)
    call = scripted(fake, users, rms, clones, [(8, MOVE, b"bobby attic", 3)])   # the den's last user; its clone record stays: two are not there
    got = r.act_many([(8, MOVE, b"bobby attic", 3)], **{**KW, "min_private_users": 2})
    assert outcomes(call) == [G.ACT_MOVED] and got.returned_public.tolist() == [True] and call["cleared"] == [2]
    assert int(r._room_rec[2, 21]) == G.PUBLIC and r._go_invite[4] == -1 and r._clear[2] == 1 and r._clear_pending
    assert model_state_differences(r, users, rms) == [] and flags(r) == only("_afk_dirty", "_who_dirty", "_rooms_dirty", "_go_dirty")
    # a move that clears the target's invitation into the room entered
    users[0]["invite"] = 3
    r.update(0, invite_room=3)
    scripted(fake, users, rms, clones, [(8, MOVE, b"alice attic", 3)])
    r.act_many([(8, MOVE, b"alice attic", 3)], **KW)
    assert r._go_invite[0] == -1 and int(r._room[0]) == 3 and model_state_differences(r, users, rms) == []
    r.look_many([4])
    assert fake.calls[-1][0] == "nd_roster_look" and "_table" not in passed(fake, r)   # the move's own look took it up already


def test_a_rejected_call_changes_nothing_after_an_accepted_one(fake):
    r, users, rms = seated()
    scripted(fake, users, rms, [], [(3, MUZ, b"alice", 2)])
    r.act_many([(3, MUZ, b"alice", 2)], **KW)
    state, before, calls = flags(r), mirrors(r), len(fake.calls)
    with pytest.raises(ValueError, match="event 1: com must be"):
        r.act_many([(3, MUZ, b"bobby", 2), (3, 99, b"", 1)], **KW)
    assert flags(r) == state and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before)) and len(fake.calls) == calls


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def act_run(built):
    res = child_run.run_child("device_act_child.py", "DEVICE_ACT", 300)
    print("\n[act]", json.dumps(res)[:6000])
    return res


@pytest.mark.gpu
def test_the_recorded_sessions_replay_on_the_device(act_run, model_replays):
    g = act_run["golden"]
    layouts = {name: [k.split(":")[1] for k in g if k.split(":")[0] == name] for name in SESSIONS}
    assert all(l == [sr.COMPACT, sr.SPREAD] for l in layouts.values()), layouts
    for key, part in g.items():
        doc, model = model_replays[key.split(":")[0]]
        assert part["n_mismatches"] == 0, (key, part["mismatches"])
        assert part["act"] == part["calls"] == model["act"] == act_lines(doc) and part["answered"] == model["answered"], key
        assert part["state_only"] == model["state_only"], key
        assert part["outcomes"] == {str(k): v for k, v in sorted(model["act_outcomes"].items())}, key
        assert part["comparisons"] == model["comparisons"] and part["plan_disagreements"] == 0
        assert part["capacity"] >= (257 if key.endswith(sr.SPREAD) else 8)


@pytest.mark.gpu
def test_seeded_streams_match_the_model(act_run):
    f = act_run["fuzz"]
    assert f["cases"] == [list(c) for c in cases()] and {c[0] for c in cases()} == set(CAPACITIES) == {1, 63, 64, 65, 256, 257}
    assert {c[1] for c in cases()} == set(LOOK_ROOMS) == {1, 6, 255, 256, 257} and f["events_per_call"] == list(EVENTS) + [1] == [1, 2, 64, 65, 1]
    assert f["calls"] == len(cases()) * 5 and f["events"] == len(cases()) * (sum(EVENTS) + 1)
    assert set(f["outcomes"]) == {str(o) for o in range(29)}, f["outcomes"]     # every outcome, ACT_DEFERRED among them
    assert min(f["outcomes"][str(o)] for o in (G.ACT_MOVE_PRIVATE, G.ACT_UNMUZZLE_ABOVE)) >= 5, f["outcomes"]      # no rarities
    assert f["n_bad"] == 0, f["first_bad"]


@pytest.mark.gpu
def test_get_user_edges(act_run):
    g = act_run["get_user"]
    assert g["n_bad"] == 0, g["first_bad"]
    assert list(EDGE_SLOTS) == [0, 63, 64, 255, 256] and len(GET_USER_WORDS) == 11
    # the exact match at 64 behind the substring match at 63 and the login slot 10 that holds the name; the substring match;
    # the 12-byte name; a 13-byte word; no substring once capitalised; slot 256; slot 0; nobody; oneself; a login slot is nobody
    found = [64, 64, 63, 255, -1, -1, 256, 0, -1, 5, -1]
    assert [t[1] for t in g["targets"]] == found * 3
    assert [t[0] for t in g["targets"][:11]] == [G.ACT_WOKEN if s not in (-1, 5) else G.ACT_WAKE_SELF if s == 5 else G.ACT_WAKE_NOBODY for s in found]
    assert [t[0] for t in g["targets"][11:22]] == [G.ACT_MUZZLED, G.ACT_MUZZLE_ALREADY, G.ACT_MUZZLED, G.ACT_MUZZLED, G.ACT_MUZZLE_ABSENT,
                                                  G.ACT_MUZZLE_ABSENT, G.ACT_MUZZLED, G.ACT_MUZZLED, G.ACT_MUZZLE_ABSENT, G.ACT_MUZZLE_SELF,
                                                  G.ACT_MUZZLE_ABSENT]
    assert [t[0] for t in g["targets"][22:]] == [G.ACT_MOVED, G.ACT_MOVE_ALREADY, G.ACT_MOVED, G.ACT_MOVED, G.ACT_MOVE_NOBODY, G.ACT_MOVE_NOBODY,
                                                G.ACT_MOVED, G.ACT_MOVED, G.ACT_MOVE_NOBODY, G.ACT_MOVE_SELF, G.ACT_MOVE_NOBODY]


@pytest.mark.gpu
def test_get_room_edges(act_run):
    g = act_run["get_room"]
    assert g["n_bad"] == 0, g["first_bad"]
    assert g["targets"]["255_256"] == [255, 256, 255, 3, -1, 3, 70, 299, -1]            # as tests/test_device_go.py has them
    assert g["targets"]["0_1023"] == [0, 1023, 0, 3, -1, 3, 70, -1, -1]


@pytest.mark.gpu
def test_a_second_run_gives_identical_bytes(act_run):
    assert act_run["determinism"] == {"same_on_a_second_call": True, "same_on_a_second_roster": True}


@pytest.mark.gpu
def test_act_many_meets_a_regrown_allocation(act_run):
    g = act_run["regrown"]
    assert g["small_outcome"] == G.ACT_WAKE_USAGE and g["clean_before"] and g["n_bad"] == 0, g
    assert g["big_h2d"] >= 5 * g["capacity"] + 600 * 4 and g["small_h2d"] < g["big_h2d"]


@pytest.mark.gpu
def test_one_call_at_the_limits(act_run):
    lim = act_run["limits"]
    assert (lim["capacity"], lim["look_rooms"], lim["clones"], lim["k"]) == (65536, 1024, 65536, 64)
    assert lim["n_bad"] == 0, lim["first_bad"]
    assert lim["mirror_ok"] and lim["muzzled"] == lim["want_muzzled"] == 8 and lim["seconds"] < 5
    assert lim["outcomes"] == sorted({G.ACT_MOVED, G.ACT_MUZZLED, G.ACT_UNMUZZLED, G.ACT_WOKEN, G.ACT_MOVE_SELF, G.ACT_MUZZLE_ABSENT,
                                      G.ACT_UNMUZZLE_NOT})
    # the private rooms 10 .. 15 held two users each; the one moved out leaves one behind, but in room 12, with the last clone
    assert lim["privates"] == [12]


@pytest.mark.gpu
def test_every_part_takes_seconds(act_run):
    assert set(act_run["seconds"]) == {"golden", "fuzz", "get_user", "get_room", "determinism", "regrown", "limits"}
    assert all(s < 60 for s in act_run["seconds"].values()), act_run["seconds"]
