"""``Roster.clone_many``: ``.clone``, ``.destroy``, ``.csay`` and ``.chear`` decided and composed on the device
(nuts_roster_clone and nuts_roster_clone_order of fanout.hip), and ``device.Clone``.

Host tier (unmarked): the names and numbers, Python's and the kernel's; the row widths and their static_asserts; everything
malformed is rejected before the device library loads, and a rejected call changes no mirror and no dirty flag; a call with
more ``.clone`` events than records behind the last occupied one is refused; the Python model of ``create_clone()``,
``destroy_clone()``, ``clone_say()`` and ``clone_hear()`` (``clone`` and ``clone_call`` of tests/device_clone_child.py)
reproduces every such step of the recorded sessions through ``CloneReplayer``, the actor's own bytes included; the new
recording holds every outcome; the already / maximum rule against the reference's loop, exhaustively; the deferral rule on
hand-built event lists; over a library that computes nothing, ``clone_many`` is passed exactly the mirrors whose flags were
set and leaves the mirrors as the model's state, compaction included, and a following ``relay_many`` and ``access_many`` are
passed the clone records again.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_clone_child.py, under ``timeout``), and the tests assert on its JSON.  Every comparison is byte-exact or
integer-exact.
"""
from __future__ import annotations

import itertools
import json
import re

import numpy as np
import pytest

import child_run
import session_replay as sr
from device_access_child import access_call
from device_clone_child import (CAPACITIES, EVENTS, KINDS, SESSIONS, WALK_CLONES, CloneReplayer, clone, clone_call, clone_lines, create_loop,
                                create_rule, fuzz_part, load, record_differences, walk_positions, walk_tables)
from device_go_child import ARCH, WIZ, go_user, seat, seat_clones, set_rooms
from device_rooms_child import list_room
from nuts333_amd import device, nuts_path
from test_device_go import FLAGS, FakeLibrary, clean, flags, mirrors, model_state_differences, only, passed

G = device
KW = {"max_clones": 2, "gatecrash_level": ARCH, "min_private_users": 2}
CLO, DES, SAY, HEAR = G.COM_CLONE, G.COM_DESTROY, G.COM_CSAY, G.COM_CHEAR
ALL = G.CLONE_HEAR_ALL
NAMES = ("CREATED", "DESTROYED", "SAID", "NO_ROOM", "PRIVATE", "ALREADY", "MAX", "DESTROY_NO_ROOM", "DESTROY_NOBODY", "DESTROY_LEVEL",
         "DESTROY_NONE_OWN", "DESTROY_NONE_THEIRS", "CSAY_MUZZLED", "CSAY_USAGE", "CSAY_NO_ROOM", "CSAY_NONE", "CHEAR_USAGE", "CHEAR_NO_ROOM",
         "CHEAR_NONE", "DEFERRED")


def hand_rooms() -> list:
    """drive (fixed public) - hallway - den (private) - attic; the hallway also adjoins the vault (fixed private)."""
    return [list_room(b"drive", links=[1], access=G.FIXED_PUBLIC), list_room(b"hallway", links=[0, 2, 4]),
            list_room(b"den", links=[1, 3], access=G.PRIVATE), list_room(b"attic", links=[2]),
            list_room(b"vault", links=[1], access=G.FIXED_PRIVATE)]


def hand_users() -> dict:
    return {0: go_user(0, name=b"Alice", room=1, colour=1, level=3, muzzled=0), 1: go_user(1, name=b"Bobby", room=2, muzzled=0),
            2: go_user(2, name=b"Carol", room=2, level=4, muzzled=0), 3: go_user(3, name=b"Dave", room=1, level=3, vis=0, muzzled=0),
            4: go_user(4, name=b"Erica", room=3, level=3, invite=2, ignall=1, muzzled=1), 5: go_user(5, name=None, room=1, muzzled=0),
            6: go_user(6, name=b"Prompt", room=1, login=1, muzzled=0), 7: go_user(7, name=None, room=None, muzzled=0)}


def seated(capacity=8, clones=6, **kw):
    rms, users = hand_rooms(), hand_users()
    r = device.Roster(capacity, look_rooms=len(rms), clones=clones, **kw)
    set_rooms(r, rms)
    seat(r, users)
    r.update(4, muzzled=1)
    return r, users, rms


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


# ------------------------------------------------------------------ host tier: names and input checks
def test_the_new_names_exist():
    assert (G.COM_CLONE, G.COM_DESTROY, G.COM_CSAY, G.COM_CHEAR) == (73, 74, 78, 79)
    assert [nuts_path.lib().np_command_name(c) for c in (73, 74, 78, 79)] == [b"clone", b"destroy", b"csay", b"chear"]
    assert G.CLONE_KERNELS == ("nuts_roster_clone", "nuts_roster_clone_order")
    assert not set(G.CLONE_KERNELS) & (set(G.KERNELS) | set(G.WHO_KERNELS) | set(G.ROOMS_KERNELS) | set(G.GO_KERNELS) | set(G.ACCESS_KERNELS))
    source = device.SOURCE.read_text()
    assert "nuts_roster_clone(CloneArgs a)" in source and "nuts_roster_clone_order(CloneOrderArgs a)" in source
    # a .chear that was obeyed has the clone_hear value it set for its outcome
    assert (G.CLONE_HEAR_NOTHING, G.CLONE_HEAR_SWEARS, G.CLONE_HEAR_ALL) == (0, 1, 2)
    assert [getattr(G, "CLONE_" + n) for n in NAMES] == list(range(3, 23))
    for n in ("HEAR_NOTHING", "HEAR_SWEARS", "HEAR_ALL") + NAMES:       # the kernel's constants, by the same names and numbers
        assert re.search(rf"\bkClone{n.title().replace('_', '')} = {getattr(G, 'CLONE_' + n)}\b", source), n
    assert "kComClone = 73, kComDestroy = 74, kComCsay = 78, kComChear = 79" in source
    assert (G.CLONE_HERE, G.CLONE_THERE, G.CLONE_RESET, G.CLONE_SAID_LINE, G.CLONE_REPLY, G.CLONE_NOTICE) == tuple(range(6))
    assert callable(G.Roster.clone_many) and G.Clone.__dataclass_fields__.keys() >= {
        "outcome", "target_room", "target_slot", "reset", "record", "created", "reply", "here", "there", "reset_plan", "notice", "said",
        "texts", "text_starts", "text_sizes", "timing"}
    # the shared loops are called, not copied: the new kernel's calls are spelt with its own argument struct
    assert source.count("wave_get_room(c.rooms") == 1 and source.count("wave_get_user(c.speech") == 1
    assert source.count("wave_get_room(a.rooms") == 2 and source.count("wave_get_user(a.speech") == 2
    doc = G.Roster.clone_many.__doc__
    assert all(word in doc for word in ("``.switch``", "``.myclones``", "``.allclones``", "relay_many", "remote users", "the prompt",
                                        "CLONE_DEFERRED", "decrease"))
    assert "clone_many" in G.Roster.go_many.__doc__ and "clone_many" in G.Roster.relay_many.__doc__


def test_the_row_widths_match_their_static_asserts():
    most = (G.MAX_CLONE_HERE, G.MAX_CLONE_THERE, G.MAX_CLONE_RESET, G.MAX_CLONE_REPLY, G.MAX_CLONE_NOTICE)
    assert most == (48, 66, 35, 87, 81) and G._CLONE_ROWS == (48, 68, 36, 88, 84)
    assert all(row == (m + 3) // 4 * 4 for m, row in zip(most, G._CLONE_ROWS))           # the longest text, rounded up to a multiple of 4
    source = device.SOURCE.read_text()
    assert "constexpr int kCloneHereRow = 48, kCloneThereRow = 68, kCloneResetRow = 36, kCloneReplyRow = 88, kCloneNoticeRow = 84;" in source
    assert "kCloneHereMax == 48 && kCloneThereMax == 66 && kCloneResetMax == 35 && kCloneReplyMax == 87 && kCloneNoticeMax == 81" in source
    # from the format strings, with the longest name and the longest room name
    users = {0: go_user(0, name=b"N" * 12, room=0, level=4, muzzled=0), 1: go_user(1, name=b"\n" * 12, room=1, level=3, muzzled=0)}
    rms = [list_room(b"r" * 20, links=[1], access=G.PRIVATE), list_room(b"p" * 20, links=[0])]
    clones = [(1, 0, ALL), None]
    results = [clone(users, rms, clones, 0, CLO, b"p", 2, 0, ARCH, 2), clone(users, rms, clones, 0, CLO, b"", 1, 0, ARCH, 2)]
    longest = {kind: max((len(r[kind]) for r in results if r[kind] is not None), default=0) for kind in ("here", "there", "reply")}
    assert results[0]["outcome"] == G.CLONE_CREATED and longest["here"] == 48 and longest["there"] == 66 and longest["reply"] == 87
    users[1]["name"] = b"M" + b"m" * 11                                       # a name get_user finds
    by_god = clone(users, rms, clones, 0, DES, b"r mmmmmmmmmmmm", 3, 0, ARCH, 9)
    assert by_god["outcome"] == G.CLONE_DESTROYED and by_god["returned"] and len(by_god["notice"]) == 81 and len(by_god["reset"]) == 35
    theirs = clone(users, rms, clones, 0, DES, b"p mmmmmmmmmmmm", 3, 0, ARCH, 2)
    assert theirs["outcome"] == G.CLONE_DESTROY_NONE_THEIRS and len(theirs["reply"]) == 61 <= 87
    said = clone(users, rms, [(0, 1, ALL)], 0, SAY, b"p " + b"x" * 996 + b"!", 3, 0, ARCH, 2)
    assert said["outcome"] == G.CLONE_SAID and len(said["said"]) - 999 <= device._SPEAK_SLACK and said["said"].startswith(b"Clone of NNNNNNNNNNNN exclaims: x")


@pytest.mark.parametrize("events, why", [
    ([], "empty call"), ((), "empty call"), (None, "events must be a sequence"), ("x", "events must be a sequence"),
    ([(0, b"den", 2)], "event 0: expected a \\(slot, com, inpstr, word_count\\) tuple"), ([[0, CLO, b"den", 2]], "event 0: expected"),
    ([(0, CLO, b"", 1), (8, CLO, b"", 1)], "event 1: slot"), ([(True, CLO, b"", 1)], "event 0: slot"),
    ([(0, 72, b"", 1)], "event 0: com must be"), ([(0, 75, b"", 1)], "event 0: com must be"), ([(0, 80, b"", 1)], "event 0: com must be"),
    ([(0, G.COM_GO, b"den", 2)], "event 0: com must be"), ([(0, True, b"", 1)], "event 0: com must be"), ([(0, None, b"", 1)], "event 0: com must be"),
    ([(0, CLO, 5, 2)], "event 0: inpstr|event 0: text"), ([(0, SAY, b"a\0b", 2)], "event 0: text contains a NUL"),
    ([(0, SAY, b"x" * 1000, 2)], "event 0: inpstr of 1000 bytes"), ([(0, DES, b"den", 11)], "event 0: word_count"),
    ([(0, DES, b"den", -1)], "event 0: word_count"), ([(0, HEAR, b"den all", None)], "event 0: word_count"),
    ([(0, CLO, b"", 1), (5, CLO, b"", 1)], "event 1: the actor, slot 5, has no name"),
    ([(6, CLO, b"", 1)], "event 0: the actor, slot 6, is still logging in"), ([(7, CLO, b"", 1)], "event 0: the actor, slot 7, is in no room"),
])
def test_malformed_events_are_rejected_before_the_library_loads(no_library, events, why):
    r, _, _ = seated()
    clean(r)
    before = mirrors(r)
    with pytest.raises(ValueError, match=why):
        r.clone_many(events, **KW)
    assert flags(r) == (False,) * len(FLAGS) and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))


@pytest.mark.parametrize("kw, why", [
    ({"gatecrash_level": 5}, "gatecrash_level"), ({"gatecrash_level": -1}, "gatecrash_level"), ({"gatecrash_level": True}, "gatecrash_level"),
    ({"gatecrash_level": "ARCH"}, "gatecrash_level"), ({"min_private_users": -1}, "min_private_users"), ({"min_private_users": 2.0}, "min_private_users"),
    ({"min_private_users": 2**31}, "min_private_users"), ({"min_private_users": None}, "min_private_users"),
    ({"max_clones": -1}, "max_clones"), ({"max_clones": 2**31}, "max_clones"), ({"max_clones": False}, "max_clones"), ({"max_clones": "2"}, "max_clones"),
    ({"record": 2}, "record"), ({"record": "yes"}, "record"),
])
def test_the_settings_are_checked(no_library, kw, why):
    r, _, _ = seated()
    clean(r)
    before = mirrors(r)
    with pytest.raises(ValueError, match=why):
        r.clone_many([(0, CLO, b"", 1)], **{**KW, **kw})
    assert flags(r) == (False,) * len(FLAGS) and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))
    for missing in KW:
        with pytest.raises(TypeError):
            r.clone_many([(0, CLO, b"", 1)], **{k: v for k, v in KW.items() if k != missing})
    with pytest.raises(TypeError):
        r.clone_many([(0, CLO, b"", 1)], 2, 3, 2)                      # keyword-only


def test_a_roster_without_rooms_or_records_rings_a_closed_one_the_tail_and_the_cap(no_library, monkeypatch):
    r = device.Roster(4, clones=2)
    r.update(0, room=0, name=b"Alice")
    with pytest.raises(ValueError, match=r"no room records \(look_rooms is 0\)"):
        r.clone_many([(0, CLO, b"", 1)], **KW)
    r, _, _ = seated(clones=0)
    with pytest.raises(ValueError, match=r"no clone records \(clones is 0\)"):
        r.clone_many([(0, CLO, b"", 1)], **KW)
    r, _, _ = seated(review_rooms=4)
    with pytest.raises(ValueError, match="record: a clone may speak in any of the 5 look rooms, and the ring rooms are 0 .. 3"):
        r.clone_many([(0, SAY, b"den hi", 3)], record=True, **KW)
    r.update(1, room=5)
    with pytest.raises(ValueError, match="event 0: the actor, slot 1, is in room 5, which has no room record"):
        r.clone_many([(1, CLO, b"", 1)], **KW)
    # six records, the last occupied one is record 3: two are left behind it, whatever lies empty before it
    r.set_clones([1, 3], owner=[0, 3], room=[1, 2])
    state, before = flags(r), mirrors(r)
    with pytest.raises(ValueError, match=r"3 \.clone events, and 2 empty clone records behind the last occupied one, record 3, of 6"):
        r.clone_many([(0, CLO, b"", 1), (0, DES, b"", 1), (3, CLO, b"", 1), (0, CLO, b"den", 2)], **KW)
    bound = 12 * (324 * 2 + 36 * 2 + 3) + 16 * 12
    monkeypatch.setattr(device, "MANY_ARENA_CAP", bound - 1)
    with pytest.raises(ValueError, match=f"call too large: its variant bound is {bound} bytes.*MANY_ARENA_CAP.*split it"):
        r.clone_many([(0, CLO, b"", 1), (0, SAY, b"den", 2)], **KW)
    assert flags(r) == state and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))
    r.close()
    with pytest.raises(ValueError, match="closed"):
        r.clone_many([(0, CLO, b"", 1)], **KW)


def test_a_call_of_too_many_cells_and_one_of_too_much_text(no_library):
    """Four admit cells an event, so a quarter of the events the other event calls take; and the said line makes the
    variant bound depend on the text, so the text's own limit is checked first."""
    big = device.Roster(G.MAX_CAPACITY, look_rooms=1, clones=1)
    big.update(0, room=0, name=b"Alice")
    with pytest.raises(ValueError, match="8192 events to 65536 slots: 4 x K x capacity must be below"):
        big.clone_many([(0, SAY, b"den hi", 3)] * 8192, **KW)
    with pytest.raises(ValueError, match="event 8190: word_count"):      # 8191 events pass that check: the next one fails
        big.clone_many([(0, SAY, b"den hi", 3)] * 8190 + [(0, SAY, b"den hi", 11)], **KW)
    r, _, _ = seated()
    state, before = flags(r), mirrors(r)
    with pytest.raises(ValueError, match="call text larger than 64 MiB: split it"):
        r.clone_many([(0, SAY, b"den " + b"x" * 995, 3)] * (2**26 // 999 + 1), **KW)
    assert flags(r) == state and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before))


# ------------------------------------------------------------------ host tier: the model against the recordings
@pytest.fixture(scope="module")
def model_replays():
    return {name: (load(name), CloneReplayer(load(name)).run()) for name in SESSIONS}


def test_the_model_reproduces_every_clone_step_of_the_recorded_sessions(model_replays):
    assert len(SESSIONS) == 11 and {"reference_only/clone.json", "clones.json", "reference_only/access.json"} < set(SESSIONS)
    for name, (doc, res) in model_replays.items():
        assert res["mismatches"] == [], (name, res["mismatches"][:1])
        assert res["clone_lines"] == clone_lines(doc) > 0, name
        assert res["plan_disagreements"] == 0 and res["comparisons"] > 0 and res["plan_checks"] > 0
    # every such line is answered, but one a NEW user typed: exec_com answers that "Unknown command."
    assert [res["clone_lines"] - res["clone"] for _, res in model_replays.values()] == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert [res["clone"] for _, res in model_replays.values()] == [39, 15, 2, 8, 7, 6, 6, 6, 11, 3, 3]
    assert model_replays["reference_only/access.json"][1]["access"] == 44               # and the door steps between them still are


def test_what_the_new_recording_holds(model_replays):
    doc, res = model_replays["reference_only/clone.json"]
    assert doc["config"] == {"max_clones": 2, "ban_swearing": True, "min_private": 2, "ignore_mp_level": WIZ, "gatecrash_level": 4}
    assert [(a["level"], a["colour"]) for a in doc["accounts"][0]] == [(1, 1), (1, 0), (3, 1), (3, 0), (4, 0)]
    assert set(res["clone_outcomes"]) == set(range(G.CLONE_DEFERRED)), res["clone_outcomes"]             # every outcome but DEFERRED
    by_note = {s["note"]: s for s in doc["steps"] if s.get("note")}
    mine = lambda note: by_note[note]["recv"][by_note[note]["actor"]]
    plain = lambda text: re.sub("\x1b\\[[0-9]*m", "", text)
    assert plain(mine("a clone created here")).startswith("You whisper a haunting spell and a clone is created here.\n\r")
    # the new clone stands beside its owner and relays the two lines of its own creation to it
    assert plain(mine("a clone created here")).endswith("[ drive ]: Dave whispers a haunting spell...\n\r[ drive ]: A clone of Dave appears in a "
                                                         "swirling magical mist!\n\r")
    assert by_note["a clone created here"]["recv"]["b"] == "Dave whispers a haunting spell...\n\rA clone of Dave appears in a swirling magical mist!\n\r"
    assert by_note["created by a room prefix"]["send"] == ".clone hall"
    # .destroy with the actor standing in the clone's room: its own bytes are the reply, then the room's line
    assert plain(mine("destroy beside the clone")) == ("You whisper a sharp spell and the clone is destroyed.\n\rThe clone of Dave shimmers and "
                                                       "vanishes.\n\r")
    back = by_note["a destroy returns the room to public"]["recv"]["b"]
    assert back == "Room access returned to PUBLIC.\n\rThe clone of Eddie shimmers and vanishes.\n\r" and "Review buffer is empty." in mine("the buffer is empty")
    assert "returned" not in by_note["a destroy leaves the room private"]["recv"]["a"] and "already private" in mine("the room is still private")
    assert by_note["the GOD destroys another's clone"]["send"] == ".destroy wizroom eddie"
    # the owner stands beside the GOD: the here line, then the notice
    assert by_note["the GOD destroys another's clone"]["recv"]["e"] == ("Gail whispers a sharp spell...\n\rSYSTEM: Gail has destroyed your clone in "
                                                                        "the wizroom.\n\r")
    assert mine("the same again") == "Eddie does not have a clone the wizroom.\n\r"
    assert by_note["csay"]["recv"]["e"] == "[ lounge ]: Clone of Dave says: hello there\n\r"          # heard by a second clone in the room
    assert "asks: what is this?" in mine("csay asks") and "exclaims: look out!" in mine("csay exclaims")
    assert by_note["csay swears"]["recv"]["b"] == "Clone of Dave says: oh shit\n\r" and "Swearing is not allowed here." in mine("a say swears")
    assert by_note["chear a mis-cased word"]["send"] == ".chear lounge All" and mine("chear a mis-cased word").startswith("Usage: chear")
    assert by_note["chear nothing, then a line"]["recv"].get("d", "") == ""
    assert by_note["an invisible creator"]["recv"]["g"].startswith("A presence whispers a haunting spell...")
    assert by_note["an invisible creator"]["recv"]["b"] == "A clone of Dave appears in a swirling magical mist!\n\r"


# ------------------------------------------------------------------ host tier: the already / maximum rule
def test_the_rule_without_a_walk_is_the_references_loop():
    """Exhaustive over an owner's record lists of up to 4 records in 3 rooms and max_clones 0 .. 4: the min and the two
    counts nuts_roster_clone takes decide as ``if (u->room==rm) ... if (++cnt==max_clones)`` does."""
    cases = 0
    for n in range(5):
        for mine in itertools.product(range(3), repeat=n):
            for rm in range(3):
                for max_clones in range(5):
                    assert create_rule(list(mine), rm, max_clones) == create_loop(list(mine), rm, max_clones), (mine, rm, max_clones)
                    cases += 1
    assert cases == (1 + 3 + 9 + 27 + 81) * 3 * 5
    assert all(create_loop([1] * n, 0, 0) == "created" and create_loop([1] * n + [0], 0, 0) == "already" for n in range(5))   # 0 never refuses
    assert create_loop([1, 0], 0, 2) == "already" and create_loop([1, 2, 0], 0, 2) == "maximum" and create_loop([1], 0, 2) == "created"
    source = device.SOURCE.read_text()                                  # the kernel's statement of it, word for word
    assert "return found && (max_clones < 1 || before < max_clones) ? 1 : max_clones >= 1 && total >= max_clones ? 2 : 0;" in source


# ------------------------------------------------------------------ host tier: the deferral rule
def outcomes(call):
    return [e["outcome"] for e in call["events"]]


def call_of(users, rms, clones, events, max_clones=2, gate=ARCH, minp=2):
    return clone_call(users, rms, clones, events, max_clones, gate, minp)


def test_create_then_speak_through_it_is_deferred():
    users, rms, clones = hand_users(), hand_rooms(), [None] * 4
    call = call_of(users, rms, clones, [(0, CLO, b"attic", 2), (0, SAY, b"attic hello", 3), (3, SAY, b"attic hello", 3)])
    assert outcomes(call) == [G.CLONE_CREATED, G.CLONE_DEFERRED, G.CLONE_DEFERRED] and clones == [(0, 3, ALL), None, None, None]
    assert all(call["events"][1][kind] is None and call["events"][1]["plans"][kind] == [] for kind in KINDS)
    assert [e["created"] for e in call["events"]] == [0, -1, -1]
    again = call_of(users, rms, clones, [(0, SAY, b"attic hello", 3)])  # submitted again it is answered: a call of one never defers
    assert outcomes(again) == [G.CLONE_SAID] and again["events"][0]["said"] == b"Clone of Alice says: hello\n" and again["events"][0]["record"] == 0
    assert again["events"][0]["plans"] == {"here": [], "there": [], "reset": [], "said": [], "reply": [], "notice": []}   # Erica ignores all
    # decided against the snapshot it would have been "You do not have a clone in that room."
    assert clone(hand_users(), hand_rooms(), [None] * 4, 0, SAY, b"attic hello", 3, 2, ARCH, 2)["outcome"] == G.CLONE_CSAY_NONE


def test_a_refusal_and_a_chear_defer_nothing_and_a_repeated_actor_alone_neither():
    users, rms = hand_users(), hand_rooms()
    clones = [(0, 3, ALL), (0, 1, ALL), (3, 3, ALL), None]
    events = [(0, CLO, b"attic", 2), (0, CLO, b"drive", 2), (0, HEAR, b"attic swears", 3), (0, SAY, b"attic really?", 3), (0, DES, b"drive", 2),
              (4, SAY, b"attic x", 3), (3, SAY, b"attic look out!", 3), (0, HEAR, b"attic Nothing", 3), (1, CLO, b"den", 2), (1, CLO, b"attic", 2)]
    call = call_of(users, rms, clones, events)
    assert outcomes(call) == [G.CLONE_ALREADY, G.CLONE_MAX, G.CLONE_HEAR_SWEARS, G.CLONE_SAID, G.CLONE_DESTROY_NONE_OWN, G.CLONE_CSAY_MUZZLED,
                              G.CLONE_SAID, G.CLONE_CHEAR_USAGE, G.CLONE_PRIVATE, G.CLONE_CREATED]    # has_room_access: even from inside
    assert clones == [(0, 3, G.CLONE_HEAR_SWEARS), (0, 1, ALL), (3, 3, ALL), (1, 3, ALL)]
    assert call["events"][3]["said"] == b"Clone of Alice asks: really?\n" and call["events"][6]["said"] == b"Clone of Dave exclaims: look out!\n"
    assert [e["record"] for e in call["events"]] == [0, -1, 0, 0, -1, -1, 2, -1, -1, -1]


def test_a_destroy_defers_what_its_owner_and_its_room_are_about_and_the_records_move_down():
    users, rms = hand_users(), hand_rooms()
    clones = [(0, 2, ALL), (3, 2, ALL), (0, 3, ALL), (3, 1, ALL), None, None]
    # Carol, a GOD, destroys Alice's clone in the den: Alice's .chear and Dave's .destroy in the den wait; Dave's .clone does not
    events = [(2, DES, b"den alice", 3), (0, HEAR, b"attic nothing", 3), (3, DES, b"den", 2), (3, CLO, b"attic", 2), (3, DES, b"hall", 2)]
    call = call_of(users, rms, clones, events, max_clones=3, minp=4)
    assert outcomes(call) == [G.CLONE_DESTROYED, G.CLONE_DEFERRED, G.CLONE_DEFERRED, G.CLONE_CREATED, G.CLONE_DEFERRED]
    first = call["events"][0]
    # Bobby, Carol and Dave's clone remain: fewer than four, the den returns to public and Erica's invitation goes
    assert first["returned"] and first["reset"] == b"Room access returned to ~FGPUBLIC.\n" and call["cleared"] == [2]
    assert rms[2]["access"] == G.PUBLIC and users[4]["invite"] is None
    assert first["notice"] == b"~OLSYSTEM: ~FRCarol has destroyed your clone in the den.\n" and first["plans"]["notice"] == [0]
    assert first["plans"]["there"] == first["plans"]["reset"] == [1, 2] and first["plans"]["here"] == [1] and first["plans"]["reply"] == [2]
    assert clones == [(3, 2, ALL), (0, 3, ALL), (3, 1, ALL), (3, 3, ALL), None, None]
    assert [e["record"] for e in call["events"]][0] == 0 and call["events"][3]["created"] == 3
    # with enough remaining the room stays private
    users, rms = hand_users(), hand_rooms()
    call = call_of(users, rms, [(0, 2, ALL), (3, 2, ALL), None], [(2, DES, b"den alice", 3)], minp=3)
    assert outcomes(call) == [G.CLONE_DESTROYED] and not call["events"][0]["returned"] and rms[2]["access"] == G.PRIVATE


def test_the_decision_chain_of_one_event():
    users, rms = hand_users(), hand_rooms()
    clones = [(0, 3, ALL), (3, 4, ALL), None]
    one = lambda slot, com, inpstr=b"", max_clones=2, gate=ARCH, minp=2, wc=None: clone(
        users, rms, clones, slot, com, inpstr, 1 + len(sr.words_of(inpstr)) if wc is None else wc, max_clones, gate, minp)
    assert one(0, CLO)["reply"] == b"~FB~OLYou whisper a haunting spell and a clone is created here.\n"
    assert one(0, CLO, b"hall")["reply"] == b"~FB~OLYou whisper a haunting spell and a clone is created here.\n"        # its own room, by name
    assert one(0, CLO, b"dr")["reply"] == b"~FB~OLYou whisper a haunting spell and a clone is created in the drive.\n"
    assert one(3, CLO, b"dr")["here"] == b"~FB~OLA presence whispers a haunting spell...\n"
    assert one(3, CLO, b"dr")["there"] == b"~FB~OLA clone of Dave appears in a swirling magical mist!\n"
    assert one(0, CLO, b"nosuch")["outcome"] == G.CLONE_NO_ROOM and one(0, CLO, b"den", wc=1)["outcome"] == G.CLONE_CREATED   # word_count decides
    assert one(0, CLO, b"den", gate=4)["outcome"] == G.CLONE_PRIVATE and one(4, CLO, b"den", gate=4)["outcome"] == G.CLONE_CREATED  # invited
    assert one(0, CLO, b"vault", gate=4)["outcome"] == G.CLONE_CREATED                 # FIXED with WIZ and above
    assert one(0, CLO, b"attic")["reply"] == b"You already have a clone in the attic.\n" and one(0, CLO, b"den", max_clones=1)["outcome"] == G.CLONE_MAX
    assert one(0, CLO, b"attic", max_clones=1)["outcome"] == G.CLONE_ALREADY and one(0, CLO, b"den", max_clones=0)["outcome"] == G.CLONE_CREATED
    assert one(0, DES, b"nosuch")["outcome"] == G.CLONE_DESTROY_NO_ROOM and one(0, DES, b"attic zed")["outcome"] == G.CLONE_DESTROY_NOBODY
    assert one(0, DES, b"vault dave")["outcome"] == G.CLONE_DESTROY_LEVEL and one(0, DES, b"attic alice")["outcome"] == G.CLONE_DESTROY_LEVEL
    assert one(0, DES, b"den")["reply"] == b"You do not have a clone in the den.\n"
    assert one(2, DES, b"den dav")["reply"] == b"Dave does not have a clone the den.\n"
    got = one(2, DES, b"vault dave")
    assert (got["outcome"], got["target_slot"], got["record"], got["there"]) == (G.CLONE_DESTROYED, 3, 1, b"~FM~OLThe clone of Dave shimmers and vanishes.\n")
    assert got["here"] == b"~FM~OLCarol whispers a sharp spell...\n" and not got["returned"]       # FIXED_PRIVATE is not exactly PRIVATE
    assert one(4, SAY, b"attic hi")["outcome"] == G.CLONE_CSAY_MUZZLED and one(0, SAY, b"attic")["outcome"] == G.CLONE_CSAY_USAGE
    assert one(0, SAY, b"nosuch hi")["outcome"] == G.CLONE_CSAY_NO_ROOM and one(0, SAY, b"den hi")["outcome"] == G.CLONE_CSAY_NONE
    assert one(0, SAY, b"attic  oh shit  ")["said"] == b"Clone of Alice says: oh shit  \n"
    assert one(3, SAY, b"vault hi")["said"] == b"Clone of Dave says: hi\n"             # the owner's own name, invisible or not
    assert one(0, HEAR, b"attic")["outcome"] == G.CLONE_CHEAR_USAGE and one(0, HEAR, b"attic ALL")["outcome"] == G.CLONE_CHEAR_USAGE
    assert one(0, HEAR, b"nosuch all")["outcome"] == G.CLONE_CHEAR_NO_ROOM and one(0, HEAR, b"den all")["outcome"] == G.CLONE_CHEAR_NONE
    assert [one(0, HEAR, b"attic " + w)["outcome"] for w in (b"nothing", b"swears", b"all")] == [0, 1, 2]


def test_the_seeded_stream_of_the_model_holds_every_outcome():
    f = fuzz_part(20263, on_device=False)                               # the child's default seed
    assert set(f["outcomes"]) == {str(o) for o in range(23)}, f["outcomes"]
    assert f["returned_public"] > 0


# ------------------------------------------------------------------ the apply step, over a library that computes nothing
CLONE_MIRROR_ARGS = {13: "_table", 14: "_speech", 15: "_clones", 16: "_rooms", 17: "_go"}


class CloneFakeLibrary(FakeLibrary):
    """The go tests' library that computes nothing; ``nd_roster_clone`` answers with the next entry of ``clone_script``: per
    event ``(outcome, target_room, target_slot, record, reset)``; ``nd_roster_access`` says "Let you into where?"."""

    def __init__(self, arrays: dict):
        super().__init__(arrays)
        self.clone_script = []

    def __getattr__(self, name):
        call = super().__getattr__(name)
        if name == "nd_roster_access":
            def access_(*args):
                call(*args)
                self.arrays[args[17]][:] = G.ACCESS_LET_WHERE
                for at in (18, 19, 20):
                    self.arrays[args[at]][:] = -1
                for at in (22, 23):
                    self.arrays[args[at]][:] = 0
                return 0
            return access_
        if name != "nd_roster_clone":
            return call

        def clone_(*args):
            call(*args)
            answer = self.clone_script.pop(0)
            for col, at in enumerate((19, 20, 21, 22, 23)):
                self.arrays[args[at]][:] = [e[col] for e in answer]
            self.arrays[args[24]][:] = -1
            for at in (26, 27):
                self.arrays[args[at]][:] = 0
            return 0
        return clone_


@pytest.fixture
def fake(monkeypatch):
    arrays: dict = {}
    lib = CloneFakeLibrary(arrays)
    real = device._ptr

    def ptr(a):
        arrays[a.ctypes.data] = a
        return real(a)

    monkeypatch.setattr(device, "_ptr", ptr)
    monkeypatch.setattr(device, "_load", lambda: lib)
    return lib


def scripted(lib, users, rms, clones, events, max_clones=2, gate=ARCH, minp=2):
    call = clone_call(users, rms, clones, events, max_clones, gate, minp)
    lib.clone_script.append([(e["outcome"], e["target_room"], e["target_slot"], e["record"], int(e["returned"])) for e in call["events"]])
    return call


def test_clone_many_is_passed_exactly_the_dirty_mirrors_and_applies_the_result(fake):
    r, users, rms = seated(8, clones=6, review_rooms=5)
    clones = [(0, 2, ALL), (3, 2, ALL), (0, 3, ALL), None, None, None]
    seat_clones(r, clones)
    kw = {**KW, "max_clones": 3}
    scripted(fake, users, rms, clones, [(0, SAY, b"", 1)], 3)
    got = r.clone_many([(0, SAY, b"", 1)], **kw)
    name, args = fake.calls[-1]
    assert name == "nd_roster_clone" and args[1] == 1 and args[9:13] == (ARCH, 2, 3, 0) and args[18] is None and len(args) == 32
    assert all(args[i] == getattr(r, m).ctypes.data for i, m in CLONE_MIRROR_ARGS.items())
    assert flags(r) == only("_afk_dirty", "_udesc_dirty", "_who_dirty") and got.effective().tolist() == [] and len(fake.calls) == 1
    scripted(fake, users, rms, clones, [(0, SAY, b"x", 2)], 3)
    r.clone_many([(0, SAY, b"x", 2)], **kw)
    assert passed(fake, r) == set()                                     # nothing changed: nothing travels
    for fields, want in (({"invite_room": 1}, {"_go"}), ({"room": 1}, {"_table"}), ({"level": 3}, {"_speech"}), ({"desc": b"d"}, set()),
                         ({"afk_mesg": b"brb"}, set()), ({"last_login": 4}, set())):
        r.update(0, **fields)
        users[0].update({("invite" if f == "invite_room" else f): v for f, v in fields.items() if f in ("invite_room", "level")})
        scripted(fake, users, rms, clones, [(0, SAY, b"x", 2)], 3)
        r.clone_many([(0, SAY, b"x", 2)], **kw)
        assert passed(fake, r) == want, fields
    r.set_rooms(3, topic=b"t")
    scripted(fake, users, rms, clones, [(0, SAY, b"x", 2)], 3)
    r.clone_many([(0, SAY, b"x", 2)], **kw)
    assert passed(fake, r) == {"_rooms"} and not r._rooms_dirty
    # a .chear: the clone records alone are stale afterwards
    call = scripted(fake, users, rms, clones, [(0, HEAR, b"attic swears", 3)], 3)
    got = r.clone_many([(0, HEAR, b"attic swears", 3)], **kw)
    assert outcomes(call) == [G.CLONE_HEAR_SWEARS] and got.effective().tolist() == [0] and got.record.tolist() == [2]
    assert flags(r) == only("_afk_dirty", "_udesc_dirty", "_who_dirty", "_clones_dirty") and record_differences(r, clones) == []
    # Carol destroys Alice's clone in the den, which returns to public; Dave clones into the attic; two events wait.  The
    # records behind the destroyed one move down, and the new one with them
    r.plan_many([(b"in the den's ring\n", 2, None, 0, device.COM_SAY)], record=True)
    events = [(2, DES, b"den alice", 3), (0, HEAR, b"attic nothing", 3), (3, CLO, b"attic", 2), (3, DES, b"den", 2)]
    call = scripted(fake, users, rms, clones, events, 3, minp=4)
    got = r.clone_many(events, **{**kw, "min_private_users": 4})
    assert passed(fake, r) == {"_clones"} and fake.calls[-1][1][10] == 4
    assert outcomes(call) == got.outcome.tolist() == [G.CLONE_DESTROYED, G.CLONE_DEFERRED, G.CLONE_CREATED, G.CLONE_DEFERRED]
    assert got.reset.tolist() == [True, False, False, False] and got.created.tolist() == [-1, -1, 2, -1] and got.record.tolist()[0] == 0
    assert clones == [(3, 2, ALL), (0, 3, G.CLONE_HEAR_SWEARS), (3, 3, ALL), None, None, None] and record_differences(r, clones) == []
    assert int(r._room_rec[2, 21]) == G.PUBLIC and r._go_invite[4] == -1 and r._clear[2] == 1 and r._clear_pending
    assert model_state_differences(r, users, rms) == []
    assert flags(r) == only("_afk_dirty", "_udesc_dirty", "_who_dirty", "_clones_dirty", "_rooms_dirty", "_go_dirty")
    # a following relay_many is passed the clone records again, and an access_many after another change of theirs
    r.relay_many([(b"a line\n", 3, None, 0, device.COM_SAY)])
    assert fake.calls[-1][0] == "nd_roster_relay" and "_clones" in passed(fake, r) and not r._clones_dirty
    call = scripted(fake, users, rms, clones, [(3, DES, b"den", 2)], 3)
    got = r.clone_many([(3, DES, b"den", 2)], **kw)
    assert outcomes(call) == [G.CLONE_DESTROYED] and got.reset.tolist() == [False] and passed(fake, r) == {"_rooms", "_go"}
    assert clones == [(0, 3, G.CLONE_HEAR_SWEARS), (3, 3, ALL), None, None, None, None] and record_differences(r, clones) == []
    r.access_many([(0, G.COM_LETMEIN, b"", 1)], gatecrash_level=ARCH, min_private_users=2, ignore_mp_level=WIZ)
    assert fake.calls[-1][0] == "nd_roster_access" and passed(fake, r) == {"_clones"}


def test_a_recording_call_passes_the_pending_clears(fake):
    r, users, rms = seated(8, clones=2, review_rooms=5)
    clones = [(0, 3, ALL), None]
    seat_clones(r, clones)
    r.clear_review([3])
    scripted(fake, users, rms, clones, [(0, SAY, b"attic hello", 3)])
    r.clone_many([(0, SAY, b"attic hello", 3)], record=True, **KW)
    args = fake.calls[-1][1]
    assert args[12] == 1 and fake.arrays[args[18]].tolist() == [0, 0, 0, 1, 0] and not r._clear_pending and not r._clear.any()


def test_a_record_that_lay_empty_before_the_call_keeps_its_place(fake):
    r, users, rms = seated(clones=7)
    clones = [(0, 3, ALL), None, (3, 3, ALL), None, (3, 0, ALL), None, None]
    seat_clones(r, clones)
    scripted(fake, users, rms, clones, [(0, HEAR, b"attic nothing", 3)])
    r.clone_many([(0, HEAR, b"attic nothing", 3)], **KW)                # nothing destroyed: nothing moves
    assert clones == [(0, 3, G.CLONE_HEAR_NOTHING), None, (3, 3, ALL), None, (3, 0, ALL), None, None] and record_differences(r, clones) == []
    events = [(3, DES, b"attic", 2), (0, CLO, b"den", 2), (1, CLO, b"attic", 2)]
    call = scripted(fake, users, rms, clones, events)
    got = r.clone_many(events, **KW)
    assert outcomes(call) == [G.CLONE_DESTROYED, G.CLONE_CREATED, G.CLONE_DEFERRED] and got.created.tolist() == [-1, 4, -1]
    assert clones == [(0, 3, G.CLONE_HEAR_NOTHING), None, None, (3, 0, ALL), (0, 2, ALL), None, None] and record_differences(r, clones) == []


def test_a_rejected_call_changes_nothing_after_an_accepted_one(fake):
    r, users, rms = seated()
    clones = [None] * 6
    scripted(fake, users, rms, clones, [(0, CLO, b"attic", 2)])
    r.clone_many([(0, CLO, b"attic", 2)], **KW)
    assert record_differences(r, clones) == [] and clones[0] == (0, 3, ALL)
    state, before, calls = flags(r), mirrors(r), len(fake.calls)
    with pytest.raises(ValueError, match="event 1: com must be"):
        r.clone_many([(0, DES, b"attic", 2), (1, 99, b"", 1)], **KW)
    assert flags(r) == state and all(np.array_equal(a, b) for a, b in zip(mirrors(r), before)) and len(fake.calls) == calls


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def clone_run(built):
    res = child_run.run_child("device_clone_child.py", "DEVICE_CLONE", 300)
    print("\n[clone]", json.dumps(res)[:6000])
    return res


@pytest.mark.gpu
def test_the_recorded_sessions_replay_on_the_device(clone_run, model_replays):
    g = clone_run["golden"]
    layouts = {name: [k.split(":")[1] for k in g if k.split(":")[0] == name] for name in SESSIONS}
    assert all(l == [sr.COMPACT, sr.SPREAD] for l in layouts.values()), layouts
    for key, part in g.items():
        doc, model = model_replays[key.split(":")[0]]
        assert part["n_mismatches"] == 0, (key, part["mismatches"])
        assert part["clone"] == part["calls"] == model["clone"] and part["clone_lines"] == clone_lines(doc), key
        assert part["access"] == model["access"] and part["go"] == model["go"], key
        assert part["outcomes"] == {str(k): v for k, v in sorted(model["clone_outcomes"].items())}, key
        assert part["plan_disagreements"] == 0 and part["plan_checks"] == model["plan_checks"], key
        assert part["comparisons"] == model["comparisons"] and part["capacity"] >= (257 if key.endswith(sr.SPREAD) else 8)


@pytest.mark.gpu
def test_seeded_streams_match_the_model(clone_run):
    f = clone_run["fuzz"]
    assert f["capacities"] == list(CAPACITIES) == [1, 64, 65, 257] and f["events_per_call"] == list(EVENTS) == [1, 8, 64]
    assert f["calls"] == 2 * len(CAPACITIES) * len(EVENTS)
    assert set(f["outcomes"]) == {str(o) for o in range(23)}, f["outcomes"]     # every outcome, CLONE_DEFERRED among them
    assert f == {**fuzz_part(20263, on_device=False), "n_bad": 0, "first_bad": []}, f["first_bad"]


@pytest.mark.gpu
def test_the_record_walk_and_the_head_count_at_the_edges(clone_run):
    w = clone_run["walk"]
    assert list(WALK_CLONES) == [1, 63, 64, 65, 255, 256, 257]
    assert walk_positions(257) == [0, 62, 63, 64, 65, 254, 255, 256] and walk_positions(64) == [0, 62, 63] and walk_positions(1) == [0]
    # what the kernel was given: Roster.clones of each table, the records filled, the cases run on it.  A full table of each
    # size for .destroy, .csay and .chear; for .clone, which needs an empty record behind the last occupied one, that size
    # with its last record empty and the next size with that many filled
    assert [t[:2] for t in w["tables"]] == [list(t) for t in walk_tables()]
    assert {t[0] for t in w["tables"] if t[0] == t[1]} == set(WALK_CLONES) <= {t[0] for t in w["tables"] if t[0] > t[1]}
    assert [t[2] for t in w["tables"]] == [5 * max(1, len(walk_positions(filled))) for _, filled in walk_tables()]
    assert w["cases"] == sum(t[2] for t in w["tables"]) == 445
    assert w["n_bad"] == 0, w["first_bad"]


@pytest.mark.gpu
def test_the_same_owner_and_room_in_every_event_all_but_the_first_defer(clone_run):
    s = clone_run["same_owner"]
    assert s["outcomes"] == [G.CLONE_CREATED] + [G.CLONE_DEFERRED] * 7 and s["n_bad"] == 0, s


@pytest.mark.gpu
def test_a_second_run_gives_identical_bytes(clone_run):
    assert clone_run["determinism"] == {"same_on_a_second_call": True, "same_on_a_second_roster": True}


@pytest.mark.gpu
def test_clone_many_meets_a_regrown_allocation(clone_run):
    g = clone_run["regrown"]
    assert g["small_outcome"] == G.CLONE_CSAY_USAGE and g["clean_before"] and g["n_bad"] == 0, g
    assert g["big_h2d"] >= 5 * g["capacity"] + g["events"] * 4 and g["small_h2d"] < g["big_h2d"] and g["events"] > 300
