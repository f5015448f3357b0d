"""``Roster.access_many``: ``.public``, ``.private``, ``.letmein`` and ``.invite`` decided and composed on the device
(nuts_roster_access and nuts_roster_access_order of fanout.hip), and ``device.Access``.

Host tier (unmarked): everything malformed is rejected before the device library loads, and a rejected call changes no
mirror and no dirty flag; the Python model of ``set_room_access()``, ``letmein()`` and ``invite()`` (``access`` and
``access_call`` of tests/device_access_child.py) reproduces every such step of the recorded sessions through
``AccessReplayer``, the actor's own bytes included; the new recording holds every outcome; the deferral rule on hand-built
event lists; over a library that computes nothing, ``access_many`` is passed exactly the mirrors whose flags were set and
leaves the mirrors as the model's state, and a following ``go_many`` is passed the room table and the go mirror again; the
longest texts stay within their rows.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_access_child.py, under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import child_run
import session_replay as sr
from device_access_child import (EDGE_SLOTS, GET_USER_WORDS, SESSIONS, AccessReplayer, access, access_call, access_lines,
                                 fuzz_part, load)
from device_go_child import ARCH, CAPACITIES, EVENTS, LOOK_ROOMS, WIZ, cases, go_call, go_user, seat, seat_clones, set_rooms
from device_rooms_child import list_room
from nuts333_amd import device, nuts_path
from test_device_go import FLAGS, FakeLibrary, clean, flags, mirrors, model_state_differences, only, passed

G = device
KW = {"gatecrash_level": ARCH, "min_private_users": 2, "ignore_mp_level": WIZ}
PUB, PRIV, LET, INV = G.COM_PUBLIC, G.COM_PRIVATE, G.COM_LETMEIN, G.COM_INVITE


def hand_rooms() -> list:
    """drive (fixed public) - hallway - den (private) - attic; the hallway also adjoins the vault (fixed private)."""
    return [list_room(b"drive", links=[1], access=G.FIXED_PUBLIC), list_room(b"hallway", links=[0, 2, 4]),
            list_room(b"den", links=[1, 3], access=G.PRIVATE), list_room(b"attic", links=[2]),
            list_room(b"vault", links=[1], access=G.FIXED_PRIVATE)]


def hand_users() -> dict:
    return {0: go_user(0, name=b"Alice", room=1, colour=1), 1: go_user(1, name=b"Bobby", room=2), 2: go_user(2, name=b"Carol", room=2, level=2),
            3: go_user(3, name=b"Dave", room=1, level=3, vis=0), 4: go_user(4, name=b"Erica", room=3, invite=2, ignall=1),
            5: go_user(5, name=None, room=1), 6: go_user(6, name=b"Prompt", room=1, login=1), 7: go_user(7, name=None, room=None)}


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
    assert (G.COM_PUBLIC, G.COM_PRIVATE, G.COM_LETMEIN, G.COM_INVITE) == (16, 17, 18, 19)
    assert [nuts_path.lib().np_command_name(c) for c in range(16, 20)] == [b"public", b"private", b"letmein", b"invite"]
    assert G.ACCESS_KERNELS == ("nuts_roster_access", "nuts_roster_access_order")
    assert not set(G.ACCESS_KERNELS) & (set(G.KERNELS) | set(G.WHO_KERNELS) | set(G.ROOMS_KERNELS) | set(G.GO_KERNELS))
    source = device.SOURCE.read_text()
    assert "nuts_roster_access(AccessArgs a)" in source and "nuts_roster_access_order(AccessOrderArgs a)" in source
    names = ("SET_PRIVATE", "SET_PUBLIC", "INVITED", "ASKED", "LOW_LEVEL", "NO_ROOM", "FIXED", "ALREADY_PUBLIC", "ALREADY_PRIVATE", "TOO_FEW",
             "LET_WHERE", "LET_NO_ROOM", "LET_ALREADY", "LET_NOT_ADJOINED", "LET_PUBLIC", "INVITE_WHO", "INVITE_PUBLIC", "INVITE_NOBODY",
             "INVITE_SELF", "INVITE_HERE", "INVITE_ALREADY", "DEFERRED")
    assert [getattr(G, "ACCESS_" + n) for n in names] == list(range(22))
    for n in names:                                                     # the kernel's constants, by the same names and numbers
        assert f"kAcc{n.title().replace('_', '')} = {getattr(G, 'ACCESS_' + n)}" in source, n
    assert (G.MAX_ACCESS_HERE, G.MAX_ACCESS_THERE, G.MAX_ACCESS_REPLY, G.MAX_ACCESS_NOTICE) == (68, 41, 83, 60)
    assert G._ACCESS_ROWS == (72, 44, 84, 60) and all(m <= row and row % 4 == 0 for m, row in zip(
        (G.MAX_ACCESS_HERE, G.MAX_ACCESS_THERE, G.MAX_ACCESS_REPLY, G.MAX_ACCESS_NOTICE), G._ACCESS_ROWS))
    assert "constexpr int kAccHereRow = 72, kAccThereRow = 44, kAccReplyRow = 84, kAccNoticeRow = 60;" in source
    assert "kAccHereMax == 68 && kAccThereMax == 41 && kAccReplyMax == 83 && kAccNoticeMax == 60" in source
    assert (G.ACCESS_HERE, G.ACCESS_THERE, G.ACCESS_REPLY, G.ACCESS_NOTICE) == (0, 1, 2, 3)
    assert callable(G.Roster.access_many) and G.Access.__dataclass_fields__.keys() >= {
        "outcome", "target_room", "target_slot", "reply", "here", "there", "notice", "texts", "text_starts", "text_sizes"}
    # the shared loops: each written once, called from the old kernel and the new one
    assert source.count("wave_get_room(a.rooms") == 2 and source.count("wave_get_user(a.speech") == 2
    doc = G.Roster.access_many.__doc__
    assert all(word in doc for word in ("``.topic``", "``.move``", "relay_many", "remote users", "the prompt", "ACCESS_DEFERRED"))
    assert "access_many" in G.Roster.go_many.__doc__


@pytest.mark.parametrize("events, why", [
    ([], "empty call"), ((), "empty call"), (None, "events must be a sequence"), ("x", "events must be a sequence"),
    ([(0, b"den", 2)], "event 0: expected a \\(slot, com, inpstr, word_count\\) tuple"), ([[0, PRIV, b"den", 2]], "event 0: expected"),
    ([(0, PRIV, b"", 1), (8, PRIV, b"", 1)], "event 1: slot"), ([(True, PRIV, b"", 1)], "event 0: slot"),
    ([(0, 15, b"", 1)], "event 0: com must be"), ([(0, 20, b"", 1)], "event 0: com must be"), ([(0, G.COM_GO, b"den", 2)], "event 0: com must be"),
    ([(0, True, b"", 1)], "event 0: com must be"), ([(0, None, b"", 1)], "event 0: com must be"),
    ([(0, PRIV, 5, 2)], "event 0: inpstr|event 0: text"), ([(0, PRIV, b"a\0b", 2)], "event 0: text contains a NUL"),
    ([(0, PRIV, b"x" * 1000, 2)], "event 0: inpstr of 1000 bytes"), ([(0, LET, b"den", 11)], "event 0: word_count"),
    ([(0, LET, b"den", -1)], "event 0: word_count"), ([(0, INV, b"bobby", None)], "event 0: word_count"),
    ([(0, PRIV, b"", 1), (5, PRIV, b"", 1)], "event 1: the actor, slot 5, has no name"),
    ([(6, PRIV, b"", 1)], "event 0: the actor, slot 6, is still logging in"), ([(7, PRIV, b"", 1)], "event 0: the actor, slot 7, is in no room"),
])
def test_malformed_events_are_rejected_before_the_library_loads(no_library, events, why):
    r, _, _ = seated()
    clean(r)
    before = mirrors(r)
    with pytest.raises(ValueError, match=why):
        r.access_many(events, **KW)
    assert flags(r) == (False,) * len(FLAGS) and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))


@pytest.mark.parametrize("kw, why", [
    ({"gatecrash_level": 5}, "gatecrash_level"), ({"gatecrash_level": -1}, "gatecrash_level"), ({"gatecrash_level": True}, "gatecrash_level"),
    ({"gatecrash_level": "ARCH"}, "gatecrash_level"), ({"min_private_users": -1}, "min_private_users"), ({"min_private_users": 2.0}, "min_private_users"),
    ({"min_private_users": 2**31}, "min_private_users"), ({"min_private_users": None}, "min_private_users"),
    ({"ignore_mp_level": 6}, "ignore_mp_level"), ({"ignore_mp_level": -1}, "ignore_mp_level"), ({"ignore_mp_level": False}, "ignore_mp_level"),
    ({"ignore_mp_level": "WIZ"}, "ignore_mp_level"),
])
def test_the_three_settings_are_checked(no_library, kw, why):
    r, _, _ = seated()
    clean(r)
    before = mirrors(r)
    with pytest.raises(ValueError, match=why):
        r.access_many([(0, PRIV, b"", 1)], **{**KW, **kw})
    assert flags(r) == (False,) * len(FLAGS) and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))
    for missing in ("gatecrash_level", "min_private_users", "ignore_mp_level"):
        with pytest.raises(TypeError):
            r.access_many([(0, PRIV, b"", 1)], **{k: v for k, v in KW.items() if k != missing})
    with pytest.raises(TypeError):
        r.access_many([(0, PRIV, b"", 1)], 3, 2, 2)                    # keyword-only


def test_a_roster_without_rooms_a_room_without_a_record_a_closed_one_and_a_call_past_the_cap(no_library, monkeypatch):
    r = device.Roster(4)
    r.update(0, room=0, name=b"Alice")
    with pytest.raises(ValueError, match=r"no room records \(look_rooms is 0\)"):
        r.access_many([(0, PRIV, b"", 1)], **KW)
    r, _, _ = seated()
    r.update(1, room=5)
    with pytest.raises(ValueError, match="event 0: the actor, slot 1, is in room 5, which has no room record"):
        r.access_many([(1, PRIV, b"", 1)], **KW)
    state, before = flags(r), mirrors(r)
    bound = 12 * 260 * 2 + 16 * 8
    monkeypatch.setattr(device, "MANY_ARENA_CAP", bound - 1)
    with pytest.raises(ValueError, match=f"call too large: its variant bound is {bound} bytes.*MANY_ARENA_CAP.*split it"):
        r.access_many([(0, PRIV, b"", 1), (0, PUB, b"", 1)], **KW)
    assert flags(r) == state and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))
    r.close()
    with pytest.raises(ValueError, match="closed"):
        r.access_many([(0, PRIV, b"", 1)], **KW)


# ------------------------------------------------------------------ host tier: the model against the recordings
@pytest.fixture(scope="module")
def model_replays():
    return {name: (load(name), AccessReplayer(load(name)).run()) for name in SESSIONS}


def test_the_model_reproduces_every_door_step_of_the_recorded_sessions(model_replays):
    for name, (doc, res) in model_replays.items():
        assert res["mismatches"] == [], (name, res["mismatches"][:1])
        assert res["access"] == res["access_lines"] == access_lines(doc) > 0, name     # none is left out
        assert res["plan_disagreements"] == 0 and res["comparisons"] > 0
    assert [res["access"] for _, res in model_replays.values()] == [44, 2, 1]
    assert model_replays["reference_only/go.json"][1]["go"] == 27                        # and the .go steps between them still are


def test_what_the_new_recording_holds(model_replays):
    doc, res = model_replays["reference_only/access.json"]
    assert doc["config"] == {"max_clones": 1, "min_private": 2, "ignore_mp_level": WIZ, "gatecrash_level": ARCH}
    assert [(a["level"], a["colour"]) for a in doc["accounts"][0]] == [(1, 1), (1, 0), (2, 0), (3, 1), (1, 0)]
    assert set(res["access_outcomes"]) == set(range(G.ACCESS_DEFERRED)), res["access_outcomes"]          # every outcome but DEFERRED
    assert 60 <= sum(1 for s in doc["steps"] if s["op"] == "line") <= 110 and res["state_only"] == 0
    by_note = {s["note"]: s for s in doc["steps"] if s.get("note")}
    mine = lambda note: by_note[note]["recv"][by_note[note]["actor"]]
    assert mine("a USER alone is refused") == "You need at least 2 users/clones in a room before it can be made private.\x1b[0m\n\r\x1b[0m"
    assert "Room set to PRIVATE" in mine("the WIZ alone is allowed") and "PRIVATE" in mine("a USER beside a clone: the clone counts")
    relayed = by_note["a USER beside a clone: the clone counts"]["recv"]["d"]           # the owner stands in the drive
    assert relayed == "\x1b[36m[ corridor ]:\x1b[0m Alice has set the room to \x1b[31mPRIVATE.\x1b[0m\n\r\x1b[0m"
    assert by_note["public again beside the clone"]["recv"]["d"].startswith("\x1b[36m[ corridor ]:")  # relayed from a private room
    assert by_note["an invisible actor"]["recv"]["b"] == "A presence has set the room to PRIVATE.\n\r"
    assert mine("inside the wizroom") == "This room's access is fixed.\n\r" and "That room's access is fixed." in mine("that room's access is fixed")
    lounge = by_note["the ARCH sets the lounge from the corridor"]["recv"]
    assert lounge["b"] == "This room has been set to PRIVATE.\n\r" and lounge["a"].startswith("This room has been set to \x1b[31mPRIVATE")
    assert "Review buffer is empty." in mine("the buffer is empty")
    assert mine("the invitation was cleared") == "That room is currently private, you cannot enter.\n\r"
    asked = by_note["the private corridor asked from the hallway"]
    assert asked["send"] == ".letmein co" and asked["recv"]["c"] == "Erica shouts asking to be let into the corridor.\n\r"
    assert asked["recv"]["b"] == "Erica shouts asking to be let in.\n\r" and "Erica shouts asking to be let in." in asked["recv"]["d"]
    unseen = by_note["an invisible asker"]["recv"]                       # letmein writes user->name
    assert unseen["e"] == "Dave shouts asking to be let into the wizroom.\n\r" and unseen["c"] == "Dave shouts asking to be let in.\n\r"
    assert by_note["invite by a lower-case substring"]["send"] == ".invite car"
    assert by_note["invite by a lower-case substring"]["recv"]["c"] == "Bobby has invited you into the corridor.\n\r"
    assert "A presence has invited you into the corridor." in by_note["an invisible inviter"]["recv"]["a"]
    assert by_note["the ignall user still receives the notice"]["recv"]["e"] == "A presence has invited you into the corridor.\n\r"
    assert "Access is " in mine("entering by the new invitation") and "currently private" in mine("the old invitation is gone")


# ------------------------------------------------------------------ host tier: the deferral rule
def outcomes(call):
    return [e["outcome"] for e in call["events"]]


def call_of(users, rms, events, clones=(), gate=ARCH, minp=2, ignore=WIZ):
    return access_call(users, rms, list(clones), events, gate, minp, ignore)


def test_private_then_invite_in_the_same_room_is_deferred():
    users, rms = hand_users(), hand_rooms()
    # Alice and Dave stand in the public hallway: she sets it private; her invitation from it waits for the next call
    call = call_of(users, rms, [(0, PRIV, b"", 1), (0, INV, b"bobby", 2)])
    assert outcomes(call) == [G.ACCESS_SET_PRIVATE, G.ACCESS_DEFERRED] and rms[1]["access"] == G.PRIVATE and users[1]["invite"] is None
    assert all(call["events"][1][kind] is None and call["events"][1]["plans"][kind] == [] for kind in ("here", "there", "reply", "notice"))
    again = call_of(users, rms, [(0, INV, b"bobby", 2)])                # submitted again it is answered: a call of one never defers
    assert outcomes(again) == [G.ACCESS_INVITED] and users[1]["invite"] == 1
    assert again["events"][0]["notice"] == b"Alice has invited you into the hallway.\n" and again["events"][0]["plans"]["notice"] == [1]
    # decided against the snapshot it would have been "This room is currently public.": the rule is what keeps the device exact
    assert access(hand_users(), hand_rooms(), [], 0, INV, b"bobby", 2, ARCH, 2, WIZ)["outcome"] == G.ACCESS_INVITE_PUBLIC


def test_two_invitations_of_one_user_the_second_is_deferred():
    users, rms = hand_users(), hand_rooms()
    call = call_of(users, rms, [(1, INV, b"alice", 2), (2, INV, b"ali", 2), (2, INV, b"dave", 2)])
    assert outcomes(call) == [G.ACCESS_INVITED, G.ACCESS_DEFERRED, G.ACCESS_INVITED]
    assert users[0]["invite"] == 2 and users[3]["invite"] == 2 and call["events"][2]["plans"]["notice"] == [3]
    assert outcomes(call_of(users, rms, [(2, INV, b"ali", 2)])) == [G.ACCESS_INVITE_ALREADY]


def test_a_repeated_actor_alone_defers_nothing():
    users, rms = hand_users(), hand_rooms()
    events = [(1, INV, b"alice", 2), (1, INV, b"dave", 2), (1, LET, b"attic", 2), (1, PUB, b"hall", 2), (1, INV, b"", 1)]
    call = call_of(users, rms, events)
    assert outcomes(call) == [G.ACCESS_INVITED, G.ACCESS_INVITED, G.ACCESS_LET_PUBLIC, G.ACCESS_LOW_LEVEL, G.ACCESS_INVITE_WHO]


def test_a_refusal_defers_nothing():
    users, rms = hand_users(), hand_rooms()
    events = [(1, PRIV, b"", 1), (2, PUB, b"vault", 2), (0, LET, b"den", 2), (1, INV, b"carol", 2), (0, PRIV, b"", 1), (3, LET, b"den", 2)]
    call = call_of(users, rms, events, minp=3)
    # already private; below gatecrash level; asked (nothing changes); already here; Alice and Dave are two, not three: too
    # few; Dave, invisible, asks as well and is answered
    assert outcomes(call) == [G.ACCESS_ALREADY_PRIVATE, G.ACCESS_LOW_LEVEL, G.ACCESS_ASKED, G.ACCESS_INVITE_HERE, G.ACCESS_TOO_FEW,
                              G.ACCESS_ASKED]
    assert call["events"][2]["here"] == b"Alice shouts asking to be let into the den.\n" and call["events"][2]["plans"]["here"] == [3, 5]
    assert call["events"][5]["here"] == b"Dave shouts asking to be let into the den.\n" and call["events"][5]["plans"]["there"] == [1, 2]
    assert call["events"][4]["reply"] == b"You need at least 3 users/clones in a room before it can be made private.\n"


def test_a_set_public_defers_what_its_room_is_about_and_clears_the_invitations():
    users, rms = hand_users(), hand_rooms()
    events = [(3, PUB, b"den", 2), (0, LET, b"den", 2), (1, INV, b"alice", 2), (4, LET, b"de", 2), (3, PRIV, b"vault", 2)]
    call = call_of(users, rms, events)
    assert outcomes(call) == [G.ACCESS_SET_PUBLIC, G.ACCESS_DEFERRED, G.ACCESS_DEFERRED, G.ACCESS_DEFERRED, G.ACCESS_FIXED]
    assert call["cleared"] == [2] and users[4]["invite"] is None and call["events"][0]["there"] == b"This room has been set to ~FGPUBLIC.\n"
    assert call["events"][0]["plans"] == {"here": [], "there": [1, 2], "reply": [3], "notice": []}
    assert call["events"][4]["reply"] == b"That room's access is fixed.\n"


def test_the_decision_chain_of_one_event():
    users, rms = hand_users(), hand_rooms()
    one = lambda slot, com, word=b"", wc=None, gate=ARCH, minp=2, ignore=WIZ, clones=(): access(
        users, rms, list(clones), slot, com, word, (2 if word else 1) if wc is None else wc, gate, minp, ignore)
    assert one(0, PRIV)["outcome"] == G.ACCESS_SET_PRIVATE and one(0, PRIV, minp=3)["outcome"] == G.ACCESS_TOO_FEW      # the login and nameless slots do not count
    assert one(0, PRIV, minp=3, clones=[(4, 1, 2)])["outcome"] == G.ACCESS_SET_PRIVATE                                 # a clone does
    assert one(0, PRIV, minp=3, ignore=1)["outcome"] == G.ACCESS_SET_PRIVATE and one(3, PRIV, minp=9)["outcome"] == G.ACCESS_SET_PRIVATE
    assert one(3, PRIV)["here"] == b"A presence has set the room to ~FRPRIVATE.\n" and one(0, PRIV)["here"] == b"Alice has set the room to ~FRPRIVATE.\n"
    assert one(0, PUB)["reply"] == b"This room is already public.\n" and one(3, PUB, b"attic")["reply"] == b"That room is already public.\n"
    assert one(1, PRIV)["reply"] == b"This room is already private.\n" and one(3, PRIV, b"de")["reply"] == b"That room is already private.\n"
    assert one(0, PRIV, b"den")["outcome"] == G.ACCESS_LOW_LEVEL and one(0, PRIV, b"den", gate=1)["outcome"] == G.ACCESS_ALREADY_PRIVATE
    assert one(0, PRIV, b"den", wc=1)["outcome"] == G.ACCESS_SET_PRIVATE                # word_count decides, not the word
    assert one(3, PRIV, b"nosuch")["outcome"] == G.ACCESS_NO_ROOM and one(3, PUB, b"drive")["reply"] == b"That room's access is fixed.\n"
    assert one(3, PRIV, b"attic")["there"] == b"This room has been set to ~FRPRIVATE.\n" and one(3, PRIV, b"attic", minp=5)["outcome"] == G.ACCESS_SET_PRIVATE
    assert one(0, LET)["outcome"] == G.ACCESS_LET_WHERE and one(0, LET, b"zz")["outcome"] == G.ACCESS_LET_NO_ROOM
    assert one(0, LET, b"hall")["reply"] == b"You are already in the hallway!\n" and one(0, LET, b"attic")["reply"] == b"The attic is not adjoined to here.\n"
    assert one(2, LET, b"drive")["outcome"] == G.ACCESS_LET_NOT_ADJOINED               # a WIZ is bound by the links here
    assert one(0, LET, b"drive")["reply"] == b"The drive is currently public.\n" and one(0, LET, b"vault")["outcome"] == G.ACCESS_ASKED
    assert one(3, LET, b"den")["there"] == b"Dave shouts asking to be let in.\n"
    assert one(0, INV)["outcome"] == G.ACCESS_INVITE_WHO and one(0, INV, b"bobby")["outcome"] == G.ACCESS_INVITE_PUBLIC
    assert one(1, INV, b"zed")["outcome"] == G.ACCESS_INVITE_NOBODY and one(1, INV, b"prompt")["outcome"] == G.ACCESS_INVITE_NOBODY
    assert one(1, INV, b"bob")["outcome"] == G.ACCESS_INVITE_SELF and one(1, INV, b"car")["reply"] == b"Carol is already here!\n"
    assert one(1, INV, b"erica")["reply"] == b"Erica has already been invited into here.\n"
    got = one(2, INV, b"dave")
    assert (got["outcome"], got["target_slot"], got["reply"], got["notice"]) == (G.ACCESS_INVITED, 3, b"You invite Dave in.\n",
                                                                                b"Carol has invited you into the den.\n")
    users[4]["invite"] = 3
    rms[4]["links"], users[3]["room"] = [1], 4                          # the invisible ARCH inside the fixed-private vault
    got = one(3, INV, b"eri")
    assert got["outcome"] == G.ACCESS_INVITED and got["notice"] == b"A presence has invited you into the vault.\n"


# ------------------------------------------------------------------ host tier: the bounds
def test_the_longest_texts_stay_within_their_rows():
    users = {0: go_user(0, name=b"N" * 12, room=0), 1: go_user(1, name=b"\n" * 12, room=1), 2: go_user(2, name=b"I" * 12, room=0, vis=0, level=3),
             3: go_user(3, name=b"T" * 12, room=2, invite=1)}
    rms = [list_room(b"r" * 20, links=[1]), list_room(b"p" * 20, links=[0], access=G.PRIVATE), list_room(b"t" * 20, access=G.FIXED_PRIVATE)]
    longest = {"here": 0, "there": 0, "reply": 0, "notice": 0}
    events = [(0, PRIV, b"", 1), (0, LET, b"p", 2), (1, LET, b"r", 2), (1, INV, b"N" * 12, 2), (1, INV, b"T" * 12, 2), (2, PRIV, b"", 1),
              (2, PUB, b"p", 2), (0, LET, b"r", 2), (0, LET, b"t", 2), (1, INV, b"\n" * 12, 2), (2, PRIV, b"t", 2), (0, PRIV, b"x", 2)]
    results = [access(users, rms, [], s, c, w, wc, ARCH, 2**31 - 1, WIZ) for s, c, w, wc in events]
    rms[0]["access"] = G.PRIVATE
    results += [access(users, rms, [], 0, INV, b"\n" * 12, 2, ARCH, 2, WIZ), access(users, rms, [], 0, INV, b"I" * 12, 2, ARCH, 2, WIZ)]
    for res in results:
        for kind, most, row in zip(longest, (G.MAX_ACCESS_HERE, G.MAX_ACCESS_THERE, G.MAX_ACCESS_REPLY, G.MAX_ACCESS_NOTICE), G._ACCESS_ROWS):
            text = res[kind]
            if text is None:
                continue
            longest[kind] = max(longest[kind], len(text))
            assert len(text) <= most <= row
            for c in (0, 1):
                ch = nuts_path.chunks(text, c)
                assert sum(map(len, ch)) <= device.max_bytes(most) and len(ch) <= device.MAX_WRITES
    assert longest == {"here": 68, "there": 41, "reply": 83, "notice": 60}
    assert results[0]["reply"] == b"You need at least 2147483647 users/clones in a room before it can be made private.\n"
    assert {r["outcome"] for r in results} >= {G.ACCESS_TOO_FEW, G.ACCESS_ASKED, G.ACCESS_INVITED, G.ACCESS_SET_PRIVATE, G.ACCESS_SET_PUBLIC,
                                               G.ACCESS_INVITE_ALREADY, G.ACCESS_INVITE_HERE, G.ACCESS_LET_ALREADY, G.ACCESS_LET_NOT_ADJOINED,
                                               G.ACCESS_FIXED, G.ACCESS_LOW_LEVEL}


def test_the_seeded_stream_of_the_model_holds_every_outcome():
    f = fuzz_part(20262, on_device=False)                               # the child's default seed
    assert set(f["outcomes"]) == {str(o) for o in range(22)}, f["outcomes"]


# ------------------------------------------------------------------ the apply step, over a library that computes nothing
ACCESS_MIRROR_ARGS = {12: "_table", 13: "_speech", 14: "_clones", 15: "_rooms", 16: "_go"}


class AccessFakeLibrary(FakeLibrary):
    """The go tests' library that computes nothing; ``nd_roster_access`` answers with the next entry of ``access_script``:
    per event ``(outcome, target_room, target_slot)``."""

    def __init__(self, arrays: dict):
        super().__init__(arrays)
        self.access_script = []

    def __getattr__(self, name):
        call = super().__getattr__(name)
        if name != "nd_roster_access":
            return call

        def access_(*args):
            call(*args)
            answer = self.access_script.pop(0)
            for col, at in enumerate((17, 18, 19)):
                self.arrays[args[at]][:] = [e[col] for e in answer]
            self.arrays[args[20]][:] = -1
            for at in (22, 23):
                self.arrays[args[at]][:] = 0
            return 0
        return access_


@pytest.fixture
def fake(monkeypatch):
    arrays: dict = {}
    lib = AccessFakeLibrary(arrays)
    real = device._ptr

    def ptr(a):
        arrays[a.ctypes.data] = a
        return real(a)

    monkeypatch.setattr(device, "_ptr", ptr)
    monkeypatch.setattr(device, "_load", lambda: lib)
    return lib


def scripted(lib, users, rms, clones, events, gate=ARCH, minp=2, ignore=WIZ):
    call = access_call(users, rms, clones, events, gate, minp, ignore)
    lib.access_script.append([(e["outcome"], e["target_room"], e["target_slot"]) for e in call["events"]])
    return call


def test_access_many_is_passed_exactly_the_dirty_mirrors_and_applies_the_result(fake):
    r, users, rms = seated(8, clones=2, review_rooms=3)
    clones = [(0, 2, device.CLONE_HEAR_ALL), None]
    seat_clones(r, clones)
    scripted(fake, users, rms, clones, [(0, LET, b"", 1)])
    got = r.access_many([(0, LET, b"", 1)], **KW)
    name, args = fake.calls[-1]
    assert name == "nd_roster_access" and args[1] == 1 and args[9:12] == (ARCH, 2, WIZ) and len(args) == 28
    assert all(args[i] == getattr(r, m).ctypes.data for i, m in ACCESS_MIRROR_ARGS.items())
    assert flags(r) == only("_afk_dirty", "_udesc_dirty", "_who_dirty") and got.effective().tolist() == [] and len(fake.calls) == 1
    scripted(fake, users, rms, clones, [(0, LET, b"x", 2)])
    r.access_many([(0, LET, b"x", 2)], **KW)
    assert passed(fake, r) == set()                                     # nothing changed: nothing travels
    for fields, want in (({"invite_room": 1}, {"_go"}), ({"room": 1}, {"_table"}), ({"level": 1}, {"_speech"}), ({"desc": b"d"}, set()),
                         ({"afk_mesg": b"brb"}, set()), ({"last_login": 4}, set())):
        r.update(0, **fields)
        users[0].update({("invite" if f == "invite_room" else f): v for f, v in fields.items() if f in ("invite_room", "level")})
        scripted(fake, users, rms, clones, [(0, LET, b"x", 2)])
        r.access_many([(0, LET, b"x", 2)], **KW)
        assert passed(fake, r) == want, fields
    r.set_rooms(3, topic=b"t")
    r.set_clones(1, owner=1, room=1)
    clones[1] = (1, 1, device.CLONE_HEAR_ALL)
    scripted(fake, users, rms, clones, [(0, LET, b"x", 2)])
    r.access_many([(0, LET, b"x", 2)], **KW)
    assert passed(fake, r) == {"_rooms", "_clones"} and not r._rooms_dirty and not r._clones_dirty
    # an invitation: the go mirror alone is stale afterwards
    call = scripted(fake, users, rms, clones, [(1, INV, b"alice", 2)])
    got = r.access_many([(1, INV, b"alice", 2)], **KW)
    assert outcomes(call) == [G.ACCESS_INVITED] and got.effective().tolist() == [0] and passed(fake, r) == set()
    assert flags(r) == only("_afk_dirty", "_udesc_dirty", "_who_dirty", "_go_dirty") and r._go_invite[0] == 2
    assert model_state_differences(r, users, rms) == []
    # the hallway set private: the room table alone
    scripted(fake, users, rms, clones, [(0, PRIV, b"", 1)])
    r.access_many([(0, PRIV, b"", 1)], **KW)
    assert passed(fake, r) == {"_go"} and flags(r) == only("_afk_dirty", "_udesc_dirty", "_who_dirty", "_rooms_dirty")
    assert int(r._room_rec[1, 21]) == G.PRIVATE and model_state_differences(r, users, rms) == []
    # the den set public by Dave from the hallway: Alice's and Erica's invitations go, and the den's ring
    r.plan_many([(b"in the den's ring\n", 2, None, 0, device.COM_SAY)], record=True)
    call = scripted(fake, users, rms, clones, [(3, PUB, b"den", 2), (1, INV, b"erica", 2)])
    got = r.access_many([(3, PUB, b"den", 2), (1, INV, b"erica", 2)], **KW)
    assert outcomes(call) == got.outcome.tolist() == [G.ACCESS_SET_PUBLIC, G.ACCESS_DEFERRED]
    assert int(r._room_rec[2, 21]) == G.PUBLIC and r._go_invite[0] == -1 and r._go_invite[4] == -1 and r._clear[2] == 1 and r._clear_pending
    assert model_state_differences(r, users, rms) == [] and flags(r) == only("_afk_dirty", "_udesc_dirty", "_who_dirty", "_rooms_dirty", "_go_dirty")
    # a following go_many is passed the room table and the go mirror again, and nothing else
    gocall = go_call(users, rms, clones, [(0, b"", 1)], ARCH, 2)
    fake.script.append([(e["outcome"], e["target"], e["old"], int(e["returned"])) for e in gocall["events"]])
    r.go_many([(0, b"", 1)], gatecrash_level=ARCH, min_private_users=2)
    assert fake.calls[-1][0] == "nd_roster_go" and passed(fake, r) == {"_rooms", "_go"}
    # and a look after a set private is passed the room table
    scripted(fake, users, rms, clones, [(1, PRIV, b"", 1)])
    r.access_many([(1, PRIV, b"", 1)], **KW)
    r.look_many([0])
    assert "_rooms" in passed(fake, r) and int(r._room_rec[2, 21]) == G.PRIVATE


def test_a_rejected_call_changes_nothing_after_an_accepted_one(fake):
    r, users, rms = seated()
    scripted(fake, users, rms, [], [(1, INV, b"alice", 2)])
    r.access_many([(1, INV, b"alice", 2)], **KW)
    state, before, calls = flags(r), mirrors(r), len(fake.calls)
    with pytest.raises(ValueError, match="event 1: com must be"):
        r.access_many([(1, INV, b"dave", 2), (1, 99, b"", 1)], **KW)
    assert flags(r) == state and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before)) and len(fake.calls) == calls


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def access_run(built):
    res = child_run.run_child("device_access_child.py", "DEVICE_ACCESS", 300)
    print("\n[access]", json.dumps(res)[:6000])
    return res


@pytest.mark.gpu
def test_the_recorded_sessions_replay_on_the_device(access_run, model_replays):
    g = access_run["golden"]
    layouts = {name: [k.split(":")[1] for k in g if k.split(":")[0] == name] for name in SESSIONS}
    assert all(l == [sr.COMPACT, sr.SPREAD] for l in layouts.values()), layouts
    for key, part in g.items():
        doc, model = model_replays[key.split(":")[0]]
        assert part["n_mismatches"] == 0, (key, part["mismatches"])
        assert part["access"] == part["calls"] == model["access"] == access_lines(doc) and part["go"] == model["go"], key
        assert part["outcomes"] == {str(k): v for k, v in sorted(model["access_outcomes"].items())}, key
        assert part["comparisons"] == model["comparisons"] and part["capacity"] >= (257 if key.endswith(sr.SPREAD) else 8)


@pytest.mark.gpu
def test_seeded_streams_match_the_model(access_run):
    f = access_run["fuzz"]
    assert f["cases"] == [list(c) for c in cases()] and {c[0] for c in cases()} == set(CAPACITIES) == {1, 63, 64, 65, 256, 257}
    assert {c[1] for c in cases()} == set(LOOK_ROOMS) == {1, 6, 255, 256, 257} and f["events_per_call"] == list(EVENTS) == [1, 2, 64, 65]
    assert f["calls"] == len(cases()) * len(EVENTS) and f["events"] == len(cases()) * sum(EVENTS)
    assert set(f["outcomes"]) == {str(o) for o in range(22)}, f["outcomes"]     # every outcome, ACCESS_DEFERRED among them
    assert f["n_bad"] == 0, f["first_bad"]


@pytest.mark.gpu
def test_head_count_edges(access_run):
    h = access_run["head_count"]
    assert h["n_bad"] == 0, h["first_bad"]
    assert list(EDGE_SLOTS) == [0, 63, 64, 255, 256]
    # the five at the edges, the actor and the clone are seven; the login slot and the nameless one are not counted, and the
    # nameless one is written to: write_room_except knows no names
    assert h["exactly_enough"] == {"outcome": G.ACCESS_SET_PRIVATE, "counted": 7, "access": G.PRIVATE, "here_to": [0, 2, 63, 64, 255, 256],
                                   "reply": "Room set to ~FRPRIVATE.\n"}
    assert h["one_fewer"] == {"outcome": G.ACCESS_TOO_FEW, "counted": 6, "access": G.PUBLIC, "here_to": [],
                              "reply": "You need at least 7 users/clones in a room before it can be made private.\n"}
    assert h["at_the_ignore_level"]["outcome"] == G.ACCESS_SET_PRIVATE and h["at_the_ignore_level"]["counted"] == 6


@pytest.mark.gpu
def test_get_user_edges(access_run):
    g = access_run["get_user"]
    assert g["n_bad"] == 0, g["first_bad"]
    assert GET_USER_WORDS == (b"anna", b"Anna", b"ann", b"abcdefghijkl", b"abcdefghijklm", b"bcdefghijkl", b"last", b"zan", b"Nna", b"host", b"prompt")
    # the exact match at 64 behind the substring match at 63 and the login slot 10 that holds the name; already invited; the
    # substring match; the 12-byte name; a 13-byte word; no substring once capitalised; slot 256; slot 0; nobody; oneself; a
    # login slot is nobody
    nobody = [G.ACCESS_INVITE_NOBODY, -1]
    assert g["targets"] == [[G.ACCESS_INVITED, 64], [G.ACCESS_INVITE_ALREADY, 64], [G.ACCESS_INVITED, 63], [G.ACCESS_INVITED, 255], nobody, nobody,
                            [G.ACCESS_INVITED, 256], [G.ACCESS_INVITED, 0], nobody, [G.ACCESS_INVITE_SELF, 5], nobody]
    assert g["invites"] == {"0": 0, "5": -1, "6": -1, "10": -1, "11": -1, "63": 0, "64": 0, "255": 0, "256": 0}


@pytest.mark.gpu
def test_get_room_edges(access_run):
    g = access_run["get_room"]
    assert g["n_bad"] == 0, g["first_bad"]
    assert g["targets"]["255_256"] == [255, 256, 255, 3, -1, 3, 70, 299, -1]            # as tests/test_device_go.py has them
    assert g["targets"]["0_1023"] == [0, 1023, 0, 3, -1, 3, 70, -1, -1]


@pytest.mark.gpu
def test_a_second_run_gives_identical_bytes(access_run):
    assert access_run["determinism"] == {"same_on_a_second_call": True, "same_on_a_second_roster": True}


@pytest.mark.gpu
def test_access_many_meets_a_regrown_allocation(access_run):
    g = access_run["regrown"]
    assert g["small_outcome"] == G.ACCESS_LET_WHERE and g["clean_before"] and g["n_bad"] == 0, g
    assert g["big_h2d"] >= 5 * g["capacity"] + 600 * 4 and g["small_h2d"] < g["big_h2d"]


@pytest.mark.gpu
def test_one_call_at_the_limits(access_run):
    lim = access_run["limits"]
    assert (lim["capacity"], lim["look_rooms"], lim["clones"], lim["k"]) == (65536, 1024, 65536, 64)
    assert lim["n_bad"] == 0, lim["first_bad"]
    assert lim["mirror_ok"] and lim["invited"] == 6
    assert set(lim["outcomes"]) >= {G.ACCESS_SET_PRIVATE, G.ACCESS_TOO_FEW, G.ACCESS_ALREADY_PRIVATE, G.ACCESS_ASKED, G.ACCESS_LET_PUBLIC,
                                    G.ACCESS_INVITED, G.ACCESS_ALREADY_PUBLIC, G.ACCESS_DEFERRED}
    # of the rooms 0 .. 9 with two users each, room 6 holds the last clone record and room 9 all the others: three are enough
    assert lim["privates"] == [6, 9, 10, 11, 12, 13, 14, 15]
    assert lim["seconds"] < 10
