"""``Roster.go_many``: ``.go`` decided and composed on the device (nuts_roster_go and nuts_roster_go_order of fanout.hip),
``device.Go``, and what ``.go`` reads of a mover, kept in a mirror of its own (``Roster.update(in_phrase=, out_phrase=,
invite_room=)``).

Host tier (unmarked): everything malformed is rejected before the device library loads, and a rejected call changes no
mirror and no dirty flag; the go mirror byte for byte; the Python model of ``go()`` (``go`` and ``go_call`` of
tests/device_go_child.py) reproduces every ``.go`` step of the recorded sessions through ``GoReplayer``, the mover's own
bytes included; the deferral rule on hand-built event lists; over a library that computes nothing, ``go_many`` is passed
exactly the mirrors whose flags were set and leaves the mirrors as the model's state, also interleaved with the other
calls; the longest texts stay within their slots on the CPU restatement; a ``Go`` built by hand obeys its contract.  The
kernels' scratch-free compile is tests/test_device_fanout.py's, which looks at every function of fanout.hip.

GPU tier: everything that touches the device runs in ONE short-lived child for the module (tests/device_go_child.py,
under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import child_run
import session_replay as sr
from device_go_child import (ARCH, CAPACITIES, EVENTS, LOOK_ROOMS, MOVED, POPULATION_SLOTS, SESSIONS, GoReplayer, cases, go, go_call,
                             go_lines, go_user, load, seat, seat_clones, set_rooms)
from device_rooms_child import list_room
from event_checks import digest as digest_of
from event_checks import event_differences
from nuts333_amd import device, nuts_path

FLAGS = ("_dirty", "_speech_dirty", "_private_dirty", "_afk_dirty", "_rooms_dirty", "_udesc_dirty", "_who_dirty", "_clones_dirty",
         "_go_dirty")
MIRRORS = ("_table", "_speech", "_rooms", "_udesc", "_who", "_afk", "_clones", "_go")
G = device


def flags(r):
    return tuple(getattr(r, f) for f in FLAGS)


def only(*names):
    return tuple(f in names for f in FLAGS)


def clean(r):
    for f in FLAGS:
        setattr(r, f, False)


def mirrors(r):
    return [getattr(r, m).copy() for m in MIRRORS]


def hand_rooms() -> list:
    """drive - hallway - den (private) - attic; the hallway has a netlink."""
    return [list_room(b"drive", links=[1]), list_room(b"hallway", links=[0, 2], netlink=(b"faraway", False, device.LINK_DOWN)),
            list_room(b"den", links=[1, 3], access=device.PRIVATE), list_room(b"attic", links=[2])]


def hand_users() -> dict:
    return {0: go_user(0, name=b"Alice", room=0, colour=1), 1: go_user(1, name=b"Bobby", room=2), 2: go_user(2, name=b"Carol", room=2, level=2),
            3: go_user(3, name=b"Dave", room=1, level=3, vis=0), 4: go_user(4, name=b"Erica", room=1, invite=2, in_phrase=b"slides in",
                                                                            out_phrase=b"wanders off"),
            5: go_user(5, name=None, room=0), 6: go_user(6, name=b"Prompt", room=0, login=1), 7: go_user(7, name=None, room=None)}


def seated(capacity=8, **kw):
    rms, users = hand_rooms(), hand_users()
    r = device.Roster(capacity, look_rooms=len(rms), **kw)
    set_rooms(r, rms)
    seat(r, users)
    return r, users, rms


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


# ------------------------------------------------------------------ host tier: names and input checks
def test_the_new_names_exist():
    assert len(device.KERNELS) == 18 and device.KERNELS[-1] == "nuts_roster_look"         # unchanged
    assert device.GO_KERNELS == ("nuts_roster_go", "nuts_roster_go_order")
    assert not set(device.GO_KERNELS) & (set(device.KERNELS) | set(device.WHO_KERNELS) | set(device.ROOMS_KERNELS))
    source = device.SOURCE.read_text()
    assert "nuts_roster_go(GoArgs a)" in source and "nuts_roster_go_order(GoOrderArgs a)" in source
    assert device.COM_GO == 10 and nuts_path.lib().np_command_name(device.COM_GO) == b"go"
    assert [G.GO_WALKED, G.GO_TELEPORTED, G.GO_UNSEEN, G.GO_WHERE, G.GO_NETLINK, G.GO_NO_ROOM, G.GO_ALREADY, G.GO_NOT_ADJOINED,
            G.GO_PRIVATE, G.GO_DEFERRED] == list(range(10))
    assert "kGoWalked = 0, kGoTeleported = 1, kGoUnseen = 2, kGoWhere = 3, kGoNetlink = 4, kGoNoRoom = 5, kGoAlready = 6" in source
    assert "kGoNotAdjoined = 7, kGoPrivate = 8, kGoDeferred = 9" in source
    assert (device.MAX_GO_ENTER, device.MAX_GO_LEAVE, device.MAX_GO_RESET, device.MAX_GO_REPLY) == (58, 83, 35, 50)
    assert device._GO_ROWS == (60, 84, 36, 52) and all(m <= row and row % 4 == 0 for m, row in zip(
        (device.MAX_GO_ENTER, device.MAX_GO_LEAVE, device.MAX_GO_RESET, device.MAX_GO_REPLY), device._GO_ROWS))
    assert "constexpr int kGoEnterRow = 60, kGoLeaveRow = 84, kGoResetRow = 36, kGoReplyRow = 52;" in source
    assert "kGoEnterMax == 58 && kGoLeaveMax == 83 && kGoReplyMax == 50" in source and "kGoResetMax = 35" in source
    assert (device.PHRASE_LEN, device._GO_REC) == (40, 88) and "constexpr int kGoRec = 88, kPhraseLen = 40;" in source
    assert callable(device.Roster.go_many) and device.Go.__dataclass_fields__.keys() >= {
        "outcome", "target", "old_room", "returned_public", "enter", "leave", "reset", "reply", "look", "look_index"}


@pytest.mark.parametrize("events, why", [
    ([], "empty call"), ((), "empty call"), (None, "events must be a sequence"), ("x", "events must be a sequence"),
    ([(0, b"hall")], "event 0: expected a \\(slot, inpstr, word_count\\) tuple"), ([[0, b"hall", 2]], "event 0: expected"),
    ([(0, b"hall", 2), (8, b"hall", 2)], "event 1: slot"), ([(True, b"hall", 2)], "event 0: slot"), ([(0, 5, 2)], "event 0: inpstr|event 0: text"),
    ([(0, b"a\0b", 2)], "event 0: text contains a NUL"), ([(0, b"x" * 1000, 2)], "event 0: inpstr of 1000 bytes"),
    ([(0, b"hall", 11)], "event 0: word_count"), ([(0, b"hall", -1)], "event 0: word_count"), ([(0, b"hall", None)], "event 0: word_count"),
    ([(0, b"hall", 2), (5, b"hall", 2)], "event 1: the mover, slot 5, has no name"),
    ([(6, b"hall", 2)], "event 0: the mover, slot 6, is still logging in"), ([(7, b"hall", 2)], "event 0: the mover, slot 7, is in no room"),
])
def test_malformed_events_are_rejected_before_the_library_loads(no_library, events, why):
    r, _, _ = seated()
    clean(r)
    before = mirrors(r)
    with pytest.raises(ValueError, match=why):
        r.go_many(events, gatecrash_level=ARCH, min_private_users=2)
    assert flags(r) == (False,) * len(FLAGS) and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))


@pytest.mark.parametrize("kw, why", [
    ({"gatecrash_level": 5, "min_private_users": 2}, "gatecrash_level"), ({"gatecrash_level": -1, "min_private_users": 2}, "gatecrash_level"),
    ({"gatecrash_level": True, "min_private_users": 2}, "gatecrash_level"), ({"gatecrash_level": "ARCH", "min_private_users": 2}, "gatecrash_level"),
    ({"gatecrash_level": 3, "min_private_users": -1}, "min_private_users"), ({"gatecrash_level": 3, "min_private_users": 2.0}, "min_private_users"),
    ({"gatecrash_level": 3, "min_private_users": None}, "min_private_users"),
])
def test_the_two_settings_are_checked(no_library, kw, why):
    r, _, _ = seated()
    with pytest.raises(ValueError, match=why):
        r.go_many([(0, b"hallway", 2)], **kw)
    for missing in ({"gatecrash_level": 3}, {"min_private_users": 2}, {}):
        with pytest.raises(TypeError):
            r.go_many([(0, b"hallway", 2)], **missing)
    with pytest.raises(TypeError):
        r.go_many([(0, b"hallway", 2)], 3, 2)                          # keyword-only


def test_a_roster_without_rooms_a_room_without_a_record_a_closed_one_and_a_call_past_the_cap(no_library, monkeypatch):
    r = device.Roster(4)
    r.update(0, room=0, name=b"Alice")
    with pytest.raises(ValueError, match=r"no room records \(look_rooms is 0\)"):
        r.go_many([(0, b"x", 2)], gatecrash_level=3, min_private_users=2)
    r, _, _ = seated()
    r.update(1, room=4)
    with pytest.raises(ValueError, match="event 0: the mover, slot 1, is in room 4, which has no room record"):
        r.go_many([(1, b"x", 2)], gatecrash_level=3, min_private_users=2)
    state, before = flags(r), mirrors(r)
    bound = 12 * 232 * 2 + 16 * 8
    monkeypatch.setattr(device, "MANY_ARENA_CAP", bound - 1)
    with pytest.raises(ValueError, match=f"call too large: its variant bound is {bound} bytes.*MANY_ARENA_CAP.*split it"):
        r.go_many([(0, b"x", 2), (0, b"y", 2)], gatecrash_level=3, min_private_users=2)
    assert flags(r) == state and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))
    r.close()
    with pytest.raises(ValueError, match="closed"):
        r.go_many([(0, b"x", 2)], gatecrash_level=3, min_private_users=2)
    with pytest.raises(ValueError, match="closed"):
        r.update(0, in_phrase=b"x")


# ------------------------------------------------------------------ host tier: the mirror
def test_the_go_mirror_byte_for_byte(no_library):
    r = device.Roster(3, look_rooms=2)
    fresh = np.zeros(88, dtype=np.uint8)
    fresh[:6], fresh[40], fresh[41:45], fresh[81], fresh[84:88] = list(b"enters"), 6, list(b"goes"), 4, 0xff
    assert r._go.shape == (3, 88) and all(np.array_equal(row, fresh) for row in r._go) and r._go_dirty
    clean(r)
    r.update([0, 2], in_phrase=[b"p" * 40, ""], out_phrase="wanders ~FRoff", invite_room=[1, None])
    assert flags(r) == only("_go_dirty")                               # these fields alone mark no other mirror
    row = r._go[0]
    assert row[:40].tobytes() == b"p" * 40 and row[40] == 40 and row[41:55].tobytes() == b"wanders ~FRoff" and row[81] == 14
    assert not row[55:81].any() and not row[82:84].any() and row[84:88].view("<i4")[0] == 1
    assert r._go[2, 40] == 0 and not r._go[2, :40].any() and r._go[2, 84:88].view("<i4")[0] == -1 and np.array_equal(r._go[1], fresh)
    assert r._go_invite.tolist() == [1, -1, -1] and np.shares_memory(r._go_invite, r._go)
    r.update([1, 1], in_phrase=[b"first", b"last"], invite_room=[0, 1])                    # the last value of a slot given twice wins
    assert r._go[1, :5].tobytes() == b"last\0" and r._go[1, 40] == 4 and r._go_invite[1] == 1
    r.update(1, in_phrase=b"x")                                        # a shorter phrase leaves nothing of the longer behind
    assert r._go[1, :4].tobytes() == b"x\0\0\0" and r._go[1, 41:45].tobytes() == b"goes"
    clean(r)
    r.update(0, invite_room=None, name=b"Zed")
    assert flags(r) == only("_go_dirty", "_speech_dirty")


@pytest.mark.parametrize("fields, why", [
    ({"in_phrase": b"p" * 41}, "in_phrase must be 0 .. 40 bytes"), ({"out_phrase": b"a\0"}, "out_phrase must be 0 .. 40 bytes"),
    ({"in_phrase": 3}, "in_phrase"), ({"in_phrase": [b"a"]}, "1 values for 2"), ({"invite_room": 4}, "room 4 has no room record"),
    ({"invite_room": -1}, "has no room record"), ({"invite_room": True}, "invite_room must be None or a look room"),
    ({"invite_room": [0]}, "1 values for 2 slots"), ({"in_phrase": b"fine", "invite_room": 9}, "room 9"),
    ({"out_phrase": b"fine", "level": 9}, "level"),
])
def test_a_rejected_update_changes_nothing(no_library, fields, why):
    r, _, _ = seated()
    clean(r)
    before = mirrors(r)
    with pytest.raises(ValueError, match=why):
        r.update([0, 1], **fields)
    assert flags(r) == (False,) * len(FLAGS) and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))


# ------------------------------------------------------------------ host tier: the model against the recordings
@pytest.fixture(scope="module")
def model_replays():
    return {name: (load(name), GoReplayer(load(name)).run()) for name in SESSIONS}


def test_the_model_reproduces_every_go_step_of_the_recorded_sessions(model_replays):
    total = 0
    for name, (doc, res) in model_replays.items():
        assert res["mismatches"] == [], (name, res["mismatches"][:1])
        # none is left out: a .go line either runs go() or, typed by a NEW user, is exec_com's "Unknown command."
        assert res["go"] + res["go_not_dispatched"] == go_lines(doc) > 0, name
        assert res["plan_disagreements"] == 0 and res["comparisons"] > 0
        total += res["go"]
    assert total == 27 + 12 + 3 + 2 + 1 + sum(res["go"] for name, (_, res) in model_replays.items() if "replay_" in name)
    assert sum(res["go_not_dispatched"] for _, res in model_replays.values()) == 5


def test_what_the_new_recording_holds(model_replays):
    doc, res = model_replays["reference_only/go.json"]
    assert doc["config"]["min_private"] == 2 and doc["config"]["gatecrash_level"] == ARCH
    assert res["go_outcomes"] == {"0": 17, "1": 1, "2": 1, "3": 1, "4": 1, "5": 1, "6": 1, "7": 1, "8": 3} and res["go"] == 27
    assert res["commands"]["private"] == res["commands"]["invite"] == res["commands"]["review"] == 1 and res["state_only"] == 0
    by_note = {s["note"]: s for s in doc["steps"] if s.get("note")}
    mine = lambda note: by_note[note]["recv"][by_note[note]["actor"]]
    assert "PRIVATE" in mine("a room made private by two users")
    for note in ("a USER refused entry; the prefix of two rooms resolves to the first", "the invitation is gone", "a USER is kept out"):
        assert mine(note) == "That room is currently private, you cannot enter.\n\r"
    for note in ("entry by invitation", "an ARCH gatecrashes", "a WIZ enters the fixed-private room", "a USER walks in", "an invisible mover"):
        assert "Access is " in mine(note)
    invited = by_note["entry by invitation"]["recv"]
    assert invited["a"] == "Erica slides \x1b[32min\x1b[0m.\x1b[0m\n\r\x1b[0m" and invited["b"] == "Erica slides in.\n\r"     # custom phrases
    assert "Erica wanders off to the hallway." in by_note["two stay behind: the room stays private"]["recv"]["b"]
    assert not any("Room access returned" in v for v in by_note["two stay behind: the room stays private"]["recv"].values())
    assert "lounge" in mine("a WIZ's teleport") and "Access is " in mine("a WIZ's teleport")       # nobody stood at either end
    stays = by_note["a user and a clone stay behind: still private"]
    assert not any("Room access returned" in v for v in stays["recv"].values())
    back = by_note["the clone alone stays behind: the room returns to public, and the clone relays it"]
    assert back["recv"]["d"].endswith("\x1b[36m[ corridor ]:\x1b[0m Room access returned to \x1b[32mPUBLIC.\x1b[0m\n\r\x1b[0m")
    # move_user looks before reset_access runs: the mover's look still shows the room it left in red
    assert "\x1b[31mcorridor" in back["recv"]["a"] and "PRIVATE" not in back["recv"]["a"]
    assert "Review buffer is empty." in mine("empty: reset_access cleared the buffer")
    assert "A presence enters the room..." in "".join(by_note["an invisible mover"]["recv"].values())
    assert "Room: " in mine("from the lounge: the corridor, not the corner") and "corridor" in mine("from the lounge: the corridor, not the corner")
    assert mine("a 45-byte word") == "There is no such room.\n\r" and len(by_note["a 45-byte word"]["send"]) == 4 + 45
    assert "netlink is inactive" in mine("the netlink branch: the link is unconnected")


# ------------------------------------------------------------------ host tier: the deferral rule
def outcomes(call):
    return [e["outcome"] for e in call["events"]]


def test_a_duplicate_slot_is_deferred():
    users, rms = hand_users(), hand_rooms()
    call = go_call(users, rms, [], [(0, b"hallway", 2), (0, b"drive", 2), (0, b"nowhere", 2)], ARCH, 2)
    assert outcomes(call) == [G.GO_WALKED, G.GO_DEFERRED, G.GO_DEFERRED] and users[0]["room"] == 1 and call["movers"] == [0]
    assert all(call["events"][1][kind] is None for kind in ("enter", "leave", "reset", "reply"))


def test_entering_the_room_another_leaves_is_deferred():
    users, rms = hand_users(), hand_rooms()
    # Alice enters the hallway; Erica, who stands there, leaves it for the den she is invited into: deferred
    call = go_call(users, rms, [], [(0, b"hallway", 2), (4, b"den", 2)], ARCH, 2)
    assert outcomes(call) == [G.GO_WALKED, G.GO_DEFERRED] and users[4]["room"] == 1 and users[4]["invite"] == 2
    again = go_call(users, rms, [], [(4, b"den", 2)], ARCH, 2)          # submitted again, it is answered: a call of one never defers
    assert outcomes(again) == [G.GO_WALKED] and users[4]["invite"] is None and again["events"][0]["enter"] == b"Erica slides in.\n"
    assert again["events"][0]["leave"] == b"Erica wanders off to the den.\n" and again["events"][0]["plans"]["leave"] == [0, 3]


def test_a_target_whose_access_an_earlier_leave_reset_is_deferred():
    users, rms = hand_users(), hand_rooms()
    users[1]["room"] = 3                                                # Carol alone in the private den
    call = go_call(users, rms, [], [(2, b"attic", 2), (0, b"hallway", 2), (4, b"den", 2)], 4, 2)
    # Carol leaves the den, which returns to public; Alice's hallway adjoins it, so her look would differ: deferred by the
    # binding's rule; Erica's target is the den itself: deferred by the call's
    assert call["events"][0]["returned"] and call["cleared"] == [2] and rms[2]["access"] == device.PUBLIC
    assert outcomes(call) == [G.GO_WALKED, G.GO_DEFERRED, G.GO_DEFERRED] and users[4]["invite"] is None     # the reset cleared it
    assert outcomes(go_call(users, rms, [], [(0, b"hallway", 2), (4, b"den", 2)], 4, 2)) == [G.GO_WALKED, G.GO_DEFERRED]


def test_a_notice_does_not_defer_its_successors():
    users, rms = hand_users(), hand_rooms()
    events = [(0, b"attic", 2), (0, b"", 1), (0, b"dr", 2), (4, b"far", 2), (4, b"den", 2), (0, b"hallway", 2)]
    call = go_call(users, rms, [], events, ARCH, 2)
    assert outcomes(call) == [G.GO_NOT_ADJOINED, G.GO_WHERE, G.GO_ALREADY, G.GO_NETLINK, G.GO_WALKED, G.GO_DEFERRED]
    assert call["events"][0]["reply"] == b"The attic is not adjoined to here.\n" and call["events"][3]["reply"] is None
    assert call["events"][2]["reply"] == b"You are already in the drive!\n" and call["movers"] == [4]


def test_the_decision_chain_of_one_event():
    users, rms = hand_users(), hand_rooms()
    one = lambda slot, word, wc=2, gate=ARCH, minp=2: go(users, rms, [], slot, word, wc, gate, minp)
    assert one(4, b"den")["outcome"] == G.GO_WALKED and one(0, b"h")["target"] == 1 and one(0, b"  hallway now", 3)["outcome"] == G.GO_WALKED
    users[4]["invite"] = None
    assert one(4, b"den")["outcome"] == G.GO_PRIVATE and one(4, b"den", gate=1)["outcome"] == G.GO_WALKED
    assert one(3, b"den")["outcome"] == G.GO_UNSEEN and one(3, b"den", gate=4)["outcome"] == G.GO_PRIVATE          # an ARCH below GOD
    rms[2]["access"] = device.FIXED_PRIVATE
    assert one(3, b"den", gate=4)["outcome"] == G.GO_UNSEEN and one(4, b"den", gate=4)["outcome"] == G.GO_PRIVATE  # a wizroom
    assert one(2, b"drive")["outcome"] == G.GO_TELEPORTED and one(1, b"drive")["outcome"] == G.GO_NOT_ADJOINED
    assert one(4, b"faraway")["outcome"] == G.GO_NETLINK and one(4, b"f")["outcome"] == G.GO_NETLINK and one(0, b"f")["outcome"] == G.GO_NO_ROOM
    assert one(4, b"farawayx")["outcome"] == G.GO_NO_ROOM and one(0, b"hallwayx")["outcome"] == G.GO_NO_ROOM
    # reset_access: the den is exactly PRIVATE again; Bobby and Carol stand there
    rms[2]["access"] = device.PRIVATE
    assert not one(1, b"hall", minp=1)["returned"] and one(1, b"hall", minp=1)["reset"] is None and one(1, b"hall", minp=2)["returned"]
    assert one(1, b"hall", minp=2)["reset"] == b"Room access returned to ~FGPUBLIC.\n" and one(1, b"hall", minp=2, gate=0)["outcome"] == G.GO_WALKED
    clones = [(0, 2, 2), None]                                          # a clone counts
    assert not go(users, rms, clones, 1, b"hall", 2, ARCH, 2)["returned"] and go(users, rms, clones, 1, b"hall", 2, ARCH, 3)["returned"]
    rms[2]["access"] = device.FIXED_PRIVATE
    assert not one(1, b"hall", minp=9)["returned"]                      # a fixed room never returns


# ------------------------------------------------------------------ host tier: the bounds
def test_the_longest_texts_stay_within_their_slots():
    users = {0: go_user(0, name=b"N" * 12, room=0, in_phrase=b"\n" * 40, out_phrase=b"\n" * 40, level=2),
             1: go_user(1, name=b"\n" * 12, room=0, level=2), 2: go_user(2, name=b"I" * 12, room=0, vis=0)}
    rms = [list_room(b"\n" * 20, links=[1], access=device.PRIVATE), list_room(b"r" * 20, links=[0]), list_room(b"t" * 20)]
    longest = {"enter": 0, "leave": 0, "reset": 0, "reply": 0}
    events = [(0, b"r", 2), (0, b"t", 2), (1, b"t", 2), (2, b"r", 2), (0, b"\n", 2), (0, b"", 1), (0, b"zz", 2), (1, b"r", 2)]
    results = [go(users, rms, [], s, w, wc, ARCH, 9) for s, w, wc in events]
    users[0]["level"] = 0
    rms[1]["access"] = device.PRIVATE
    results += [go(users, rms, [], 0, b"t", 2, ARCH, 9), go(users, rms, [], 0, b"r", 2, ARCH, 9), go(users, rms, [], 0, b"\n" * 20, 2, ARCH, 9)]
    for res in results:
        for kind, most, row in zip(longest, (G.MAX_GO_ENTER, G.MAX_GO_LEAVE, G.MAX_GO_RESET, G.MAX_GO_REPLY), G._GO_ROWS):
            text = res[kind]
            if text is None:
                continue
            longest[kind] = max(longest[kind], len(text))
            assert len(text) <= most <= row
            for c in (0, 1):
                ch = nuts_path.chunks(text, c)
                assert sum(map(len, ch)) <= device.max_bytes(most) and len(ch) <= device.MAX_WRITES
    assert longest == {"enter": 58, "leave": 83, "reset": 35, "reply": 50}
    assert {r["outcome"] for r in results} >= {G.GO_WALKED, G.GO_TELEPORTED, G.GO_UNSEEN, G.GO_ALREADY, G.GO_WHERE, G.GO_NO_ROOM,
                                               G.GO_NOT_ADJOINED, G.GO_PRIVATE}


# ------------------------------------------------------------------ the dataclass
def hand_built_go():
    """A Go from the model alone: one call over hand_users(), texts and variants scattered over buffers of 0xAA bytes."""
    users, rms = hand_users(), hand_rooms()
    events = [(3, b"far", 2), (0, b"", 1), (2, b"drive", 2), (4, b"den", 2), (1, b"attic", 2)]
    colour = {j: u["colour"] for j, u in users.items()}
    call = go_call(users, rms, [], events, ARCH, 2)
    k, cap = len(events), 8
    texts, variants = np.full(2000, 0xAA, dtype=np.uint8), np.full(20_000, 0xAA, dtype=np.uint8)
    tstarts, tsizes = np.zeros((4, k), dtype=np.int64), np.full((4, k), -1, dtype=np.int64)
    starts, sizes = np.zeros((4, k, 2), dtype=np.int64), np.zeros((4, k, 2), dtype=np.int64)
    counts, wsz = np.zeros((4, k, 2), dtype=np.int32), np.full((4, k, 2, device.MAX_WRITES), -7, dtype=np.int32)
    bits = np.zeros((4, k, 1), dtype=np.uint64)
    at, vat = 3, 7
    for b, res in enumerate(call["events"]):
        for row, kind in enumerate(("enter", "leave", "reset", "reply")):
            text = res[kind]
            if text is None:
                continue
            tstarts[row, b], tsizes[row, b] = at, len(text)
            texts[at:at + len(text)] = np.frombuffer(text, dtype=np.uint8)
            at += len(text) + 5
            bits[row, b, 0] = sum(1 << j for j in res["plans"][kind])
            for c in (0, 1):
                ch = nuts_path.chunks(text, c)
                data = b"".join(ch)
                starts[row, b, c], sizes[row, b, c], counts[row, b, c] = vat, len(data), len(ch)
                variants[vat:vat + len(data)] = np.frombuffer(data, dtype=np.uint8)
                wsz[row, b, c, :len(ch)] = [len(x) for x in ch]
                vat += len(data) + 3
    colour_bits = device._pack(np.array([bool(colour.get(j, 0)) for j in range(cap)]))
    plans = [device.Plan(capacity=cap, admitted_bits=bits[i], colour_bits=colour_bits, variants=variants, variant_starts=starts[i],
                         variant_sizes=sizes[i], write_counts=counts[i], write_sizes=wsz[i]) for i in range(4)]
    got = device.Go(outcome=np.array(outcomes(call), dtype=np.int8), target=np.array([e["target"] for e in call["events"]], dtype=np.int32),
                    old_room=np.array([e["old"] for e in call["events"]], dtype=np.int32),
                    returned_public=np.array([e["returned"] for e in call["events"]]), enter=plans[0], leave=plans[1], reset=plans[2],
                    reply=plans[3], texts=texts, text_starts=tstarts, text_sizes=tsizes, look_index=np.array([-1, -1, 0, -1, -1], dtype=np.int32))
    return got, call


def test_a_hand_built_go_obeys_the_contract(no_library):
    got, call = hand_built_go()
    assert outcomes(call) == [G.GO_NETLINK, G.GO_WHERE, G.GO_TELEPORTED, G.GO_DEFERRED, G.GO_DEFERRED]
    assert got.moved().tolist() == [2] and got.timing == {} and got.look is None and got.returned_public.tolist() == [False, False, True, False, False]
    assert got.leave_text(2) == b"~FT~OLCarol chants a spell and vanishes into a magical blue vortex!\n"
    assert got.reply_text(1) == b"Go where?\n" and got.reply.recipients(1, 1).tolist() == [0] and got.reply.recipients(1, 0).tolist() == []
    # the drive's Alice and its nameless slot (write_room_except knows no names); the den's Bobby
    assert got.enter.admitted(2).nonzero()[0].tolist() == [0, 5] and got.leave.admitted(2).nonzero()[0].tolist() == [1]
    for b in (0, 3, 4):                                                 # a netlink and a deferred event have no text at all
        for plan, text in ((got.enter, got.enter_text), (got.leave, got.leave_text), (got.reset, got.reset_text), (got.reply, got.reply_text)):
            assert text(b) == b"" and not plan.admitted(b).any() and plan.chunks(b, 0) == plan.chunks(b, 1) == []
    assert got.enter_text(2).startswith(b"~FT~OLCarol appears") and got.enter.chunks(2, 1)[-1] == b"\x1b[0m"
    assert got.reset_text(2) == b"Room access returned to ~FGPUBLIC.\n" and got.reset.admitted(2).nonzero()[0].tolist() == [1]
    assert got.reset_text(1) == b"" and got.reply_text(2) == b"" and got.enter_text(1) == b""
    for call_ in (got.enter_text, got.leave_text, got.reset_text, got.reply_text):
        for bad in (-1, 5):
            with pytest.raises(IndexError):
                call_(bad)
    with pytest.raises(IndexError):
        got.enter.chunks(0, 2)


# ------------------------------------------------------------------ the apply step, over a library that computes nothing
GO_MIRROR_ARGS = {10: "_table", 11: "_speech", 12: "_clones", 13: "_rooms", 14: "_go"}


class FakeLibrary:
    """Every ``nd_roster_*`` call returns 0 and is kept in ``calls`` as ``(name, args)``; ``nd_roster_go`` answers with the
    next entry of ``script``: per event ``(outcome, target, old_room, returned)``."""

    def __init__(self, arrays: dict):
        self.calls, self.arrays, self.script = [], arrays, []
        self._buffer = np.zeros(16, dtype=np.uint8)

    def nd_arena(self):
        return self._buffer.ctypes.data

    nd_write_sizes = nd_arena

    def nd_last_error(self):
        return b"the fake library has no errors"

    def __getattr__(self, name):
        if not name.startswith("nd_roster_"):
            raise AttributeError(name)

        def call(*args):
            if name in ("nd_roster_create", "nd_roster_destroy", "nd_roster_review_rooms", "nd_roster_revtell_rings",
                        "nd_roster_look_rooms", "nd_roster_clones"):
                return 0
            self.calls.append((name, args))
            if name == "nd_roster_tell":
                self.arrays[args[15]][:] = -1
                self.arrays[args[16]][:] = -1
            if name == "nd_roster_go":
                answer = self.script.pop(0)
                for col, at in enumerate((15, 16, 17, 18)):
                    self.arrays[args[at]][:] = [e[col] for e in answer]
                self.arrays[args[19]][:] = -1
                for at in (21, 22):
                    self.arrays[args[at]][:] = 0
            return 0
        return call


@pytest.fixture
def fake(monkeypatch):
    arrays: dict = {}
    lib = FakeLibrary(arrays)
    real = device._ptr

    def ptr(a):
        arrays[a.ctypes.data] = a
        return real(a)

    monkeypatch.setattr(device, "_ptr", ptr)
    monkeypatch.setattr(device, "_load", lambda: lib)
    return lib


def passed(lib, r, which=-1) -> set:
    """The mirrors of ``r`` a library call was handed."""
    name, args = lib.calls[which]
    ints = {a for a in args if isinstance(a, int) and not isinstance(a, bool)}
    return {m for m in MIRRORS if getattr(r, m).size and getattr(r, m).ctypes.data in ints}


def scripted(lib, users, rms, clones, events, gate=ARCH, minp=2):
    """The model's call, and its answers queued for the fake library."""
    call = go_call(users, rms, clones, events, gate, minp)
    lib.script.append([(e["outcome"], e["target"], e["old"], int(e["returned"])) for e in call["events"]])
    return call


def model_state_differences(r, users, rms) -> list:
    bad = [("room", j) for j, u in users.items() if int(r._room[j]) != (-1 if u["room"] is None else u["room"])]
    bad += [("invite", j) for j, u in users.items() if int(r._go_invite[j]) != (-1 if u["invite"] is None else u["invite"])]
    return bad + [("access", i) for i, rm in enumerate(rms) if int(r._room_rec[i, 21]) != rm["access"]]


def test_go_many_is_passed_exactly_the_dirty_mirrors_and_applies_the_moves(fake):
    r, users, rms = seated(8, clones=2, review_rooms=3)
    clones = [(0, 2, device.CLONE_HEAR_ALL), None]
    seat_clones(r, clones)
    scripted(fake, users, rms, clones, [(0, b"", 1)])
    got = r.go_many([(0, b"", 1)], gatecrash_level=ARCH, min_private_users=2)
    name, args = fake.calls[-1]
    assert name == "nd_roster_go" and args[1] == 1 and args[8:10] == (ARCH, 2) and len(args) == 27
    assert all(args[i] == getattr(r, m).ctypes.data for i, m in GO_MIRROR_ARGS.items())
    assert flags(r) == only("_afk_dirty", "_udesc_dirty", "_who_dirty") and got.look is None and got.look_index.tolist() == [-1]
    assert len(fake.calls) == 1                                         # nobody moved: one device visit
    scripted(fake, users, rms, clones, [(0, b"x", 2)])
    r.go_many([(0, b"x", 2)], gatecrash_level=ARCH, min_private_users=2)
    assert passed(fake, r) == set()
    for fields, want in (({"in_phrase": b"in"}, {"_go"}), ({"invite_room": 1}, {"_go"}), ({"room": 0}, {"_table"}), ({"level": 1}, {"_speech"}),
                         ({"desc": b"d"}, set()), ({"afk_mesg": b"brb"}, set()), ({"last_login": 4}, set())):
        r.update(0, **fields)
        users[0].update({("invite" if f == "invite_room" else f): v for f, v in fields.items() if f in ("invite_room", "level")})
        scripted(fake, users, rms, clones, [(0, b"x", 2)])
        r.go_many([(0, b"x", 2)], gatecrash_level=ARCH, min_private_users=2)
        assert passed(fake, r) == want, fields
    r.set_rooms(3, topic=b"t")
    r.set_clones(1, owner=1, room=1)
    clones[1] = (1, 1, device.CLONE_HEAR_ALL)
    scripted(fake, users, rms, clones, [(0, b"x", 2)])
    r.go_many([(0, b"x", 2)], gatecrash_level=ARCH, min_private_users=2)
    assert passed(fake, r) == {"_rooms", "_clones"} and not r._rooms_dirty and not r._clones_dirty
    # a move: Erica walks into the den by invitation.  The table and the go mirror are stale afterwards; the look has
    # uploaded the table already, the go mirror waits for the next go_many
    before = len(fake.calls)
    call = scripted(fake, users, rms, clones, [(4, b"den", 2)])
    got = r.go_many([(4, b"den", 2)], gatecrash_level=ARCH, min_private_users=2)
    assert [n for n, _ in fake.calls[before:]] == ["nd_roster_go", "nd_roster_look"] and passed(fake, r, before) == set()
    assert passed(fake, r) == {"_table", "_udesc"} and flags(r) == only("_afk_dirty", "_who_dirty", "_go_dirty")      # the roster's first look
    assert got.look is not None and got.look.slots.tolist() == [4] and got.look_index.tolist() == [0]
    assert model_state_differences(r, users, rms) == [] and users[4]["room"] == 2 and users[4]["invite"] is None
    # the den empties: Bobby walks out (two and a clone stay), Carol (one and the clone), then Erica: it returns to public
    r.update(1, invite_room=2)
    users[1]["invite"] = 2
    r.plan_many([(b"in the den's ring\n", 2, None, 0, device.COM_SAY)], record=True)
    for slot, returned in ((1, False), (2, False), (4, True)):
        before = len(fake.calls)
        call = scripted(fake, users, rms, clones, [(slot, b"hallway", 2)], minp=2)
        assert call["events"][0]["returned"] == returned
        r.go_many([(slot, b"hallway", 2)], gatecrash_level=ARCH, min_private_users=2)
        assert model_state_differences(r, users, rms) == []
        # the look comes before the reset: it was handed the table alone, never the room table
        assert [n for n, _ in fake.calls[before:]] == ["nd_roster_go", "nd_roster_look"] and passed(fake, r) == {"_table"}
    assert int(r._room_rec[2, 21]) == device.PUBLIC and r._go_invite[1] == -1 and r._clear[2] == 1 and r._clear_pending
    assert flags(r) == only("_afk_dirty", "_who_dirty", "_go_dirty", "_rooms_dirty")
    scripted(fake, users, rms, clones, [(0, b"x", 2)])
    r.go_many([(0, b"x", 2)], gatecrash_level=ARCH, min_private_users=2)
    assert passed(fake, r) == {"_rooms", "_go"}


def test_the_binding_defers_a_move_next_to_a_room_an_earlier_event_returned(fake):
    r, users, rms = seated(8, review_rooms=3)
    users[1]["room"] = 3
    r.update(1, room=3)
    events = [(2, b"attic", 2), (0, b"hallway", 2), (4, b"", 1)]
    call = scripted(fake, users, rms, [], events, gate=4)
    # the device's rule knows no links: it would answer Alice's move.  The model defers it, and so must the binding
    fake.script[-1][1] = (G.GO_WALKED, 1, 0, 0)
    got = r.go_many(events, gatecrash_level=4, min_private_users=2)
    assert outcomes(call) == got.outcome.tolist() == [G.GO_WALKED, G.GO_DEFERRED, G.GO_WHERE]
    assert got.look.slots.tolist() == [2] and got.look_index.tolist() == [0, -1, -1] and got.returned_public.tolist() == [True, False, False]
    assert model_state_differences(r, users, rms) == [] and int(r._room[0]) == 0


def test_go_many_interleaved_with_the_other_calls(fake):
    """No call reads a stale field after a move, and no existing call is passed more than on a roster that never went."""
    def build():
        r, users, rms = seated(8, clones=2, review_rooms=3, revtell=True)
        r.set_clones(0, owner=0, room=0, hear=2)
        return r, users, rms

    calls = {"look": lambda r: r.look_many([0, 1]), "relay": lambda r: r.relay_many([(b"hi\n", 0, 1, 0, 3)]),
             "tell": lambda r: r.tell_many([(0, device.COM_TELL, b"bobby psst", 3)]),
             "speak": lambda r: r.speak_many([(0, device.COM_SAY, b"hello", 1)]),
             "who": lambda r: r.who_many([0, 1], now=5, date=b"DATE"), "rooms": lambda r: r.rooms_many([0, 1], topics=[True, False])}
    reads = {"look": {"_table", "_speech", "_rooms", "_udesc"}, "relay": {"_table", "_clones"}, "tell": {"_table", "_speech", "_afk"},
             "speak": {"_table", "_speech"}, "who": {"_table", "_speech", "_rooms", "_udesc", "_who"}, "rooms": {"_table", "_speech", "_rooms"},
             "go": {"_table", "_speech", "_clones", "_rooms", "_go"}}
    r, users, rms = build()
    clones = [(0, 0, 2), None]
    stale = set(MIRRORS)
    walk = [(0, b"hallway"), (4, b"den"), (0, b"drive"), (4, b"hallway"), (1, b"hallway"), (2, b"hallway")]
    for n, (slot, word) in enumerate(walk * 2):
        before = len(fake.calls)
        call = scripted(fake, users, rms, clones, [(slot, word, 2)])
        r.go_many([(slot, word, 2)], gatecrash_level=ARCH, min_private_users=2)
        got = passed(fake, r, before)
        assert got <= stale and not (reads["go"] - got) & stale, (n, got, stale)
        stale -= got
        if call["movers"]:
            stale |= {"_table"}
            got = passed(fake, r, before + 1)                           # the look of the move
            assert "_table" in got and got <= stale and not (reads["look"] - got) & stale
            stale -= got
        if call["cleared"] or any(e["outcome"] in MOVED for e in call["events"]):
            stale |= {"_go"} if r._go_dirty else set()
            stale |= {"_rooms"} if r._rooms_dirty else set()
        assert model_state_differences(r, users, rms) == []
        order = list(calls)
        for kind in order[n % 6:] + order[:n % 6]:
            calls[kind](r)
            got = passed(fake, r)
            assert got <= stale and not (reads[kind] - got) & stale, (n, kind, got, stale)
            stale -= got
    assert int(r._room_rec[2, 21]) == device.PUBLIC                     # the den was emptied on the way


# ------------------------------------------------------------------ host tier: the comparison the event children share
STAND_IN_KINDS, STAND_IN_DEFERRED, STAND_IN_EFFECTIVE, STAND_IN_CAPACITY = ("here", "reply"), 9, (1,), 8


class StandInPlan:
    """What event_differences and digest read of a device.Plan, held as given."""

    def __init__(self, slots, chunks):
        self.bits = np.zeros((len(slots), STAND_IN_CAPACITY), dtype=bool)
        for k, admitted in enumerate(slots):
            self.bits[k, admitted] = True
        self.chunk_lists = chunks                                       # [k][c]: a list of bytes
        self.variant_sizes = np.array([[sum(map(len, both[c])) for c in (0, 1)] for both in chunks], dtype=np.int32)
        self.write_counts = np.array([[len(both[c]) for c in (0, 1)] for both in chunks], dtype=np.int32)

    @property
    def admitted_bits(self):
        return np.packbits(self.bits, axis=1, bitorder="little")

    def admitted(self, k):
        return self.bits[k]

    def chunks(self, k, c):
        return list(self.chunk_lists[k][c])


class StandIn:
    """A result as the event calls give one, built from a model's call: every field says what the model says."""

    def __init__(self, call):
        events = call["events"]
        self.outcome = np.array([e["outcome"] for e in events], dtype=np.int32)
        self.target = np.array([e["target"] for e in events], dtype=np.int32)
        self.held = np.zeros(len(events), dtype=bool)                   # a field a deferred event must leave alone
        self.texts = {kind: [e[kind] or b"" for e in events] for kind in STAND_IN_KINDS}
        self.text_sizes = np.array([[-1 if e[kind] is None else len(e[kind]) for e in events] for kind in STAND_IN_KINDS], dtype=np.int32)
        self.plans = {kind: StandInPlan([e["plans"][kind] for e in events],
                                        [[nuts_path.chunks(e[kind], c) if e[kind] is not None else [] for c in (0, 1)] for e in events])
                      for kind in STAND_IN_KINDS}
        self.effective_events = [k for k, e in enumerate(events) if e["outcome"] in STAND_IN_EFFECTIVE]

    def effective(self):
        return np.array(self.effective_events, dtype=np.int64)

    def kinds(self):
        return tuple((kind, self.plans[kind], lambda k, kind=kind: self.texts[kind][k]) for kind in STAND_IN_KINDS)

    def differences(self, call):
        return event_differences(self, call, self.kinds(), STAND_IN_DEFERRED, lambda k, res: ((int(self.target[k]),), (res["target"],)),
                                 also_deferred=lambda k: self.held[k], effective=STAND_IN_EFFECTIVE)

    def digest(self):
        return digest_of(self, [self.target], self.kinds())


def test_the_shared_comparison_finds_each_single_change_and_the_digest_moves():
    nothing = {"here": None, "reply": None, "plans": {"here": [], "reply": []}}
    call = {"events": [
        {"slot": 0, "com": 4, "outcome": 1, "target": 5, "here": b"~FRUaaa~RS waves.\n", "reply": b"You wave.\n",
         "plans": {"here": [1, 2, 7], "reply": [0]}},
        {"slot": 1, "com": 4, "outcome": 3, "target": -1, "here": None, "reply": b"Wave at whom?\n", "plans": {"here": [], "reply": [1]}},
        {"slot": 0, "com": 4, "outcome": STAND_IN_DEFERRED, "target": 5, **nothing}]}
    assert nuts_path.chunks(call["events"][0]["here"], 0) != nuts_path.chunks(call["events"][0]["here"], 1)
    faithful = StandIn(call)
    assert faithful.differences(call) == []

    def outcome(g): g.outcome[0] = 3
    def extra_field(g): g.target[0] = 6
    def text_byte(g): g.texts["here"][0] = g.texts["here"][0].replace(b"waves", b"wavez")
    def present_empty_text(g): g.text_sizes[0, 1] = 0                   # the text itself is b"" either way
    def admitted_slot(g): g.plans["here"].bits[0, 3] = True
    def chunk_of_colour_1(g): g.plans["reply"].chunk_lists[0][1][0] += b"!"
    def deferred_write_count(g): g.plans["reply"].write_counts[2, 1] = 1
    def deferred_variant_size(g): g.plans["here"].variant_sizes[2, 0] = 1
    def deferred_admitted_slot(g): g.plans["here"].bits[2, 0] = True
    def deferred_text_size(g): g.text_sizes[1, 2] = 0
    def deferred_own_field(g): g.held[2] = True
    def effective_list(g): g.effective_events.append(1)

    changes = ((outcome, "outcome", 0, True), (extra_field, "outcome", 0, True), (text_byte, "here text", 0, True),
               (present_empty_text, "here text", 1, True), (admitted_slot, "here plan", 0, True), (chunk_of_colour_1, "reply plan", 0, True),
               (deferred_write_count, "a deferred event", 2, False), (deferred_variant_size, "a deferred event", 2, False),
               (deferred_admitted_slot, "a deferred event", 2, True), (deferred_text_size, "a deferred event", 2, True),
               (deferred_own_field, "a deferred event", 2, False), (effective_list, "effective", None, False))
    for change, what, event, hashed in changes:
        got = StandIn(call)
        assert got.digest() == faithful.digest()
        change(got)
        bad = got.differences(call)
        assert [(b["what"], b.get("event")) for b in bad] == [(what, event)], (change.__name__, bad)
        if event is not None:
            e = call["events"][event]
            assert (bad[0]["slot"], bad[0]["com"], bad[0]["model"]) == (e["slot"], e["com"], e["outcome"]) and "device" in bad[0]
            assert ("want" in bad[0]) == (what != "a deferred event"), bad
        assert (got.digest() != faithful.digest()) == hashed, change.__name__


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def go_run(built):
    res = child_run.run_child("device_go_child.py", "DEVICE_GO", 300)
    print("\n[go]", json.dumps(res)[:6000])
    return res


@pytest.mark.gpu
def test_the_recorded_sessions_replay_on_the_device(go_run, model_replays):
    g = go_run["golden"]
    layouts = {name: [k.split(":")[1] for k in g if k.split(":")[0] == name] for name in SESSIONS}
    assert all(l == [sr.COMPACT, sr.SPREAD] for l in layouts.values()), layouts
    for key, part in g.items():
        doc, model = model_replays[key.split(":")[0]]
        assert part["n_mismatches"] == 0, (key, part["mismatches"])
        assert part["go"] == part["calls"] == model["go"] and part["go"] + part["go_not_dispatched"] == go_lines(doc), key
        assert part["outcomes"] == model["go_outcomes"] and part["comparisons"] == model["comparisons"], key
        assert part["capacity"] >= (257 if key.endswith(sr.SPREAD) else 8)


@pytest.mark.gpu
def test_seeded_streams_match_the_model(go_run):
    f = go_run["fuzz"]
    assert f["cases"] == [list(c) for c in cases()] and {c[0] for c in cases()} == set(CAPACITIES) == {1, 63, 64, 65, 256, 257}
    assert {c[1] for c in cases()} == set(LOOK_ROOMS) == {1, 6, 255, 256, 257} and f["events_per_call"] == list(EVENTS) == [1, 2, 64, 65]
    assert f["calls"] == len(cases()) * len(EVENTS) and f["events"] == len(cases()) * sum(EVENTS)
    assert set(f["outcomes"]) == {str(o) for o in range(10)}, f["outcomes"]     # every outcome, GO_DEFERRED among them
    assert f["returned_public"] > 0
    assert f["n_bad"] == 0, f["first_bad"]


@pytest.mark.gpu
def test_get_room_edges(go_run):
    g = go_run["get_room"]
    assert g["n_bad"] == 0, g["first_bad"]
    # twin, twinroom_b, twinroom_, the 20-byte name by its full length, one byte more, one byte less, a nameless room's
    # would-be name (room 7 has none: n7 is the prefix of n70), the last room, a sibling that does not exist
    assert g["targets"]["255_256"] == [255, 256, 255, 3, -1, 3, 70, 299, -1]
    assert g["targets"]["0_1023"] == [0, 1023, 0, 3, -1, 3, 70, -1, -1]        # n1023 was renamed to twinroom_b


@pytest.mark.gpu
def test_population_edges(go_run):
    p = go_run["population"]
    assert p["n_bad"] == 0, p["first_bad"]
    # slot 2, without a name, is not counted and is written to: write_room_except knows no names, as in plan_many
    assert list(POPULATION_SLOTS) == [0, 63, 64, 255, 256]
    assert p["stays_private"] == {"returned": False, "behind": 6, "reset_to": [], "access": device.PRIVATE, "guest_invite": 0, "ring_lines": 1}
    assert p["returns_public"] == {"returned": True, "behind": 6, "reset_to": [0, 2, 63, 64, 255, 256], "access": device.PUBLIC,
                                   "guest_invite": -1, "ring_lines": 0}


@pytest.mark.gpu
def test_a_second_run_gives_identical_bytes(go_run):
    assert go_run["determinism"] == {"same_on_a_second_call": True, "same_on_a_second_roster": True}


@pytest.mark.gpu
def test_go_many_meets_a_regrown_allocation(go_run):
    g = go_run["regrown"]
    assert g["small_outcome"] == device.GO_WHERE and g["clean_before"] and g["n_bad"] == 0, g
    # the table was not dirty, and travelled again from the pinned mirror: its two slices, beyond what 600 events carry
    assert g["big_h2d"] >= 5 * g["capacity"] + 600 * 4 and g["small_h2d"] < g["big_h2d"]


@pytest.mark.gpu
def test_one_call_at_the_limits(go_run):
    lim = go_run["limits"]
    assert (lim["capacity"], lim["look_rooms"], lim["clones"], lim["k"]) == (65536, 1024, 65536, 64)
    assert lim["n_bad"] == 0, lim["first_bad"]
    assert lim["mirror_ok"] and lim["looks"] >= 8 and device.GO_WALKED in lim["outcomes"]
    # every private room one of its two users left returned to public, but room 6, where the last clone record stands
    assert lim["publics"] == [0, 2, 4, 8, 10, 12, 14]
    assert lim["seconds"] < 10
