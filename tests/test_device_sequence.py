"""The sixteen device calls of ``device.Roster`` interleaved: the host mirrors and their dirty flags, the pending ring
clears, and the device allocation that is freed and made anew when a call needs more.

Host tier (unmarked): ``device._load`` is replaced by a library that computes nothing and records what it is passed.  A
seeded stream of updates, ``set_rooms``, ``set_clones``, clears and calls runs over one roster with every feature on, and
an independent model says which fields are stale on the device: an update makes its fields stale, passing a mirror to the
library cleans every field that lives in it.  After every call no field that call kind reads (``READS`` of
tests/device_sequence_child.py, from the kernels) may be stale, and a pending clear goes down with the first call that
touches its rings and with no later one.  ``go_many`` changes the mirrors itself: the fake library answers ``nd_roster_go``
from the model's ``go_call``, so the binding's apply step really runs, and the model makes stale what the model's call says
changed -- the table after a move, ``invite_room`` after a dropped invite, ``rooms.access`` and a pending review clear after
a room returned to public -- never what the roster says.  ``access_many``, ``clone_many`` and ``set_many`` likewise, answered
from ``access_call``, ``clone_call`` and ``set_call``: stale afterwards are exactly the fields in which the State differs
from what it was before the model's call (``State.changed_since``) -- an access, an invitation, the clone records that a
``.destroy`` moved down, the flags and texts of the effective ``set_many`` events, a room's topic.  What a ``set_many`` reads
depends on the call: the room's topic only when it holds a ``.topic`` (``reads_of``).  ``act_many`` is answered from
``act_call`` and is both: stale after it is what the State says changed, and when it moved somebody it looks in the middle
of its apply step as ``go_many`` does -- the table is stale before that look and clean after it, and the access of a room
returned to public, the invitations and the muzzles become stale behind it.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_sequence_child.py, under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import json
import random

import numpy as np
import pytest

import child_run
from device_sequence_child import (CAPACITIES, CLONE_FIELDS, EVENT_COUNTS, EVENT_KINDS, FIELDS, GO_TABLES, KEPT_BACK, KINDS,
                                   LOOK_ROOMS, MIRROR_OF, MIRRORS, MUZZLE_FIELDS, NOWHERE, READS, RECORDING_KINDS, RELAY_NAMES, REPLACEMENT_CAPACITY,
                                   REVIEW_ROOMS, ROOM_FIELDS, SEEDS, SET_TABLES, STEPS_PER_ROSTER, TABLE_FIELDS, TABLE_KINDS,
                                   TOPIC_READS, UNREAD, USER_FIELDS, Coverage, Runner, State, apart, clear_blocks, new_roster, op_for,
                                   random_op, reads_of, sequence_part, slice_of)
from nuts333_amd import device

HOST_STEPS = 3000
#: the least a seed's device run counts, from the model's calls: see assert_the_counts
#: (the dry run counts 140 and 139 moves, 30 and 31 rooms returned, 369 and 361 deferred events, 7,914 and 8,727 who lines, 593
#: and 610 listings)
MOVES, RETURNED, DEFERRED, WHO_LINES, ROOMS_LISTINGS = 100, 20, 200, 5000, 400
#: ... and of access_many, clone_many and set_many (EVENT_COUNTS): the dry run's count for the poorer seed, rounded down to
#: one significant figure; behind each the two seeds' counts
EVENT_FLOORS = {"access_effective": 100,      # 146, 155
                "clone_effective": 100,       # 132, 178
                "set_effective": 500,         # 544, 623
                "access_deferred": 100,       # 155, 197
                "clone_deferred": 100,        # 100, 106
                "set_deferred": 200,          # 224, 225
                "set_private": 60,            # 62, 66
                "access_returned": 50,        # 53, 59: ring rooms and others that an access_many set public
                "destroy_returned": 30,       # 33, 30
                "created": 9,                 # 9, 42: seed 20262 has one clone record on three of its five rosters
                "destroyed": 60,              # 63, 80
                "compacted": 30,              # 32, 48
                "said_recorded": 4,           # 6, 4: on the one roster of a seed where clone_many may record
                "topic_calls": 90,            # 92, 96
                "topicless_dirty": 20,        # 25, 29
                # act_many's, with the streams as act_many left them (the fifteen above hold on those too: 148 and 131, 143 and
                # 204, 671 and 703, 132 and 159, 133 and 115, 236 and 209, 60 and 62, 53 and 52, 31 and 39, 14 and 52, 68 and
                # 96, 33 and 59, 5 and 6, 95 and 94, 28 and 26)
                "act_effective": 100,         # 147, 128
                "act_deferred": 100,          # 123, 157
                "act_moved": 60,              # 72, 63
                "act_returned": 20,           # 24, 24: the six clear blocks on the four rosters of a seed that have a second slot
                "act_invites_cleared": 100,   # 112, 166
                "act_muzzled": 20,            # 34, 22
                "act_unmuzzled": 40,          # 41, 43
                "act_woken": 10,              # 30, 14
                "act_wake_afk": 3,            # 7, 3
                "act_unmuzzle_above": 20,     # 26, 28: four of them the muzzle whose bit was taken and put back
                "act_private_alone": 9}       # 9, 9: calls that passed the speaker state on _private_dirty alone
#: where each entry point takes its pending clears, and the argument that says whether it records (None: it always
#: touches the rings); nd_roster_plan and nd_roster_relay take no clears and touch no ring, and neither do nd_roster_who,
#: nd_roster_rooms and nd_roster_go, whose argument lists hold the kept tables and the results alone: the clear a go_many
#: leaves behind goes down with a later call.  nd_roster_clone carries the clear at its own position, and only when it
#: records; nd_roster_access and nd_roster_set have no such argument (None) and never carry one: the clear an access_many
#: leaves behind waits as go_many's does, and so does the one an act_many leaves: nd_roster_act has no such argument either
CLEAR_AT = {"nd_roster_plan_record": (-1, None, False), "nd_roster_relay_record": (-1, None, False),
            "nd_roster_review": (3, None, False), "nd_roster_revtell": (3, None, True), "nd_roster_speak": (13, 10, False),
            "nd_roster_input": (11, 8, False), "nd_roster_tell": (13, 9, True), "nd_roster_clone": (18, 12, False),
            "nd_roster_access": (None, None, False), "nd_roster_set": (None, None, False), "nd_roster_act": (None, None, False)}
#: how many arguments the four newest entry points take: the positions above and in FakeLibrary.ANSWERS count on it
ARGUMENTS = {"nd_roster_access": 28, "nd_roster_clone": 32, "nd_roster_set": 24, "nd_roster_act": 29}
ENTRY_POINTS = {"broadcast_many": ("nd_roster_fanout",), "plan_many": ("nd_roster_plan", "nd_roster_plan_record"),
                "speak_many": ("nd_roster_speak",), "input_many": ("nd_roster_input",), "tell_many": ("nd_roster_tell",),
                "look_many": ("nd_roster_look",), "relay_many": ("nd_roster_relay", "nd_roster_relay_record"),
                "who_many": ("nd_roster_who",), "rooms_many": ("nd_roster_rooms",), "go_many": ("nd_roster_go",),
                "access_many": ("nd_roster_access",), "clone_many": ("nd_roster_clone",), "set_many": ("nd_roster_set",), "act_many": ("nd_roster_act",),
                "review_many": ("nd_roster_review",), "revtell_many": ("nd_roster_revtell",)}


# ------------------------------------------------------------------ a library that computes nothing
class FakeLibrary:
    """Every ``nd_roster_*`` call returns 0 and is kept in ``calls`` as ``(name, args)``.  ``arrays`` maps an address
    ``device._ptr`` handed out to its array, so that what an argument points at can be looked at.  ``nd_roster_go`` answers
    with the next entry of ``script``, per event ``(outcome, target, old_room, returned)``, as the fake library of
    tests/test_device_go.py does: the Runner puts the model's there.  ``nd_roster_access``, ``nd_roster_clone`` and
    ``nd_roster_set`` answer from the same queue, as the fake libraries of their own test modules do: per event ``(outcome,
    target_room, target_slot)``, ``(outcome, target_room, target_slot, record, returned)`` and ``(outcome, has a reply2)``;
    ``nd_roster_act`` likewise, per event ``(outcome, target_slot, target_room, old_room, returned)``."""

    #: entry point -> where its per-event answers go, in the order of a script row; where clen goes; the two to zero
    ANSWERS = {"nd_roster_go": ((15, 16, 17, 18), 19, (21, 22)), "nd_roster_access": ((17, 18, 19), 20, (22, 23)),
               "nd_roster_clone": ((19, 20, 21, 22, 23), 24, (26, 27)), "nd_roster_set": ((15,), 16, (18, 19)),
               "nd_roster_act": ((16, 17, 18, 19, 20), 21, (23, 24))}

    def __init__(self, arrays: dict):
        self.calls, self.arrays, self.handles, self.script = [], arrays, 0, []
        self._buffer = np.zeros(16, dtype=np.uint8)

    def nd_roster_create(self, capacity):
        self.handles += 1
        return self.handles - 1

    def nd_arena(self):
        return self._buffer.ctypes.data

    nd_write_sizes = nd_arena

    def nd_last_error(self):
        return b"the fake library has no errors"

    def __getattr__(self, name):
        if not name.startswith("nd_roster_"):
            raise AttributeError(name)

        def call(*args):
            if name in ("nd_roster_destroy", "nd_roster_review_rooms", "nd_roster_revtell_rings", "nd_roster_look_rooms",
                        "nd_roster_clones"):
                return 0
            self.calls.append((name, args))
            if name == "nd_roster_tell":                                # tell_many indexes by what the device found
                self.arrays[args[15]][:] = -1
                self.arrays[args[16]][:] = -1
            if name in self.ANSWERS:                                    # the model's answers; no text at all
                answer = self.script.pop(0)
                columns, clen, zeroed = self.ANSWERS[name]
                assert len(answer) == args[1], f"{name}: the script's next answer is for {len(answer)} events, the call has {args[1]}"
                for col, at in enumerate(columns):
                    self.arrays[args[at]][:] = [e[col] for e in answer]
                self.arrays[args[clen]][:] = -1
                if name == "nd_roster_set":                             # the binding takes the AFK message where clen says reply2
                    self.arrays[args[clen]][device.SET_REPLY2, [k for k, e in enumerate(answer) if e[1]]] = 17
                for at in zeroed:
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


# ------------------------------------------------------------------ which fields are stale on the device
class Host(Coverage):
    """The staleness model, fed by the Runner's steps and by what the fake library was passed."""

    def __init__(self, lib: FakeLibrary, roster: device.Roster, state: State):
        super().__init__()
        self.lib, self.roster, self.state = lib, roster, state
        self.stale = set(FIELDS)                                        # nothing is on the device yet
        self.stale_at_call = set()                                      # (kind, field) with the field stale when kind was called
        self.awaiting, self.read_clean_later = set(), set()             # (kind, unread stale field) pairs, and those confirmed
        self.masks = [np.zeros(state.review_rooms, dtype=np.uint8), np.zeros(state.cap, dtype=np.uint8)]
        self.clear_pending = [False, False]
        self.clears_sent = [0, 0]
        self.step = None
        self.log = []                                                   # per library call: (kind, the mirrors it was passed)

    def updated(self, label, fields) -> None:
        super().updated(label, fields)
        self.stale |= set(fields)

    def cleared(self, label, tell, which=()) -> None:
        super().cleared(label, tell)
        self.masks[int(tell)][list(which)] = 1
        self.clear_pending[int(tell)] = True

    def names(self) -> np.ndarray:
        out = np.zeros((LOOK_ROOMS, device._RELAY_NAME_ROW), dtype=np.uint8)
        for i, rm in enumerate(self.state.rooms):
            out[i, :len(rm["name"])] = np.frombuffer(rm["name"], dtype=np.uint8)
            out[i, device.ROOM_NAME_LEN] = len(rm["name"])
        return out

    def called(self, label, kind, review_rings, revtell_rings, go=None, change=None, reads=None) -> None:
        super().called(label, kind, review_rings, revtell_rings, go, change, reads)
        calls, self.lib.calls[:] = list(self.lib.calls), []
        names = [name for name, _ in calls]
        if kind == "go_many":
            # nd_roster_go, and when somebody moved nd_roster_look over the movers: a look_many like any other.  What is stale
            # afterwards is what the model's call says changed
            assert names == ["nd_roster_go"] + ["nd_roster_look"] * go["moved"], f"{self.step}: go_many made the library calls {names}"
            self.library_call("go_many", *calls[0])
            if go["moved"]:
                self.stale |= set(TABLE_FIELDS)                         # the apply step moved them on the host
                self.library_call("look_many", *calls[1])
            if go["invites_dropped"]:
                self.stale.add("invite_room")
            if go["returned"]:
                self.stale.add("rooms.access")
                self.left_pending(go["rings"])
            touches = [False, False]
        elif kind == "act_many":
            # nd_roster_act, and when it moved somebody nd_roster_look over the moved in the middle of the apply step: the moves
            # and the invitations they clear come before that look, the rooms returned to public and the muzzles behind it
            moved = change["moved"]
            assert names == ["nd_roster_act"] + ["nd_roster_look"] * moved, f"{self.step}: act_many made the library calls {names}"
            self.library_call("act_many", *calls[0])
            assert change["stale"] <= set(FIELDS) and ("room" in change["stale"]) == moved
            if moved:
                self.stale |= set(TABLE_FIELDS)                         # the apply step moved them on the host
                self.library_call("look_many", *calls[1])
            self.stale |= change["stale"] - {"room"}
            self.left_pending(change["rings"])
            touches = [False, False]
        else:
            assert len(calls) == 1, f"{self.step}: {kind} made {len(calls)} library calls"
            assert names[0] in ENTRY_POINTS[kind], f"{self.step}: {kind} went through {names[0]}"
            self.library_call(kind, *calls[0], reads)
            touches = self.clears(*calls[0])
            if change:
                # the apply step ran on the host after the library call, and after the clear the call carried: stale is what
                # the model's call says changed, and a ring room it returned to public leaves a clear pending
                assert change["stale"] <= set(FIELDS)
                self.stale |= change["stale"]
                self.left_pending(change["rings"])
        assert touches == [bool(review_rings), bool(revtell_rings)], f"{self.step}: {names[0]} and the test disagree on the rings"
        self.lib.arrays.clear()

    def left_pending(self, rings) -> None:
        if rings:
            self.masks[0][rings] = 1
            self.clear_pending[0] = True

    def library_call(self, kind, name, args, reads=None) -> None:
        """One library call of ``kind``: the mirrors it was passed are clean, and nothing it reads may be stale.  ``reads``:
        what this call reads, where that is not READS of its kind."""
        reads = READS[kind] if reads is None else reads
        assert len(args) == ARGUMENTS.get(name, len(args)), f"{self.step}: {name} takes {len(args)} arguments"
        ints = {a for a in args if isinstance(a, int) and not isinstance(a, bool)}
        passed = {m for m in MIRRORS if device._ptr(getattr(self.roster, m)) in ints}
        want = self.names()
        if any(a in self.lib.arrays and self.lib.arrays[a].shape == want.shape and np.array_equal(self.lib.arrays[a], want)
               for a in ints):
            passed.add("names")
        self.log.append((kind, frozenset(passed)))
        before = set(self.stale)
        self.stale_at_call |= {(kind, f) for f in before}
        self.stale -= {f for f in FIELDS if MIRROR_OF[f] in passed}
        read_stale = sorted(reads & self.stale)
        assert not read_stale, (f"{self.step}: {kind} ({name}) read {read_stale} stale: it was passed {sorted(passed)}, dirty flags "
                                f"{ {f: getattr(self.roster, f) for f in ('_dirty', '_speech_dirty', '_private_dirty', '_set_dirty', '_afk_dirty', '_rooms_dirty', '_udesc_dirty', '_clones_dirty', '_who_dirty', '_go_dirty')} }")
        self.read_clean_later |= {(k, f) for k, f in self.awaiting if f in reads}
        self.awaiting |= {(kind, f) for f in before - reads}

    def clears(self, name, args) -> list:
        """The pending clears: down with the first call that records into, or reads, their rings, and with no later one.
        Returns which rings the call touches."""
        at = CLEAR_AT.get(name)
        touches = [False, False]
        if at is not None and at[0] is not None:
            where, record_at, tell = at
            if record_at is None or args[record_at]:
                touches[int(tell)] = True
                clear = args[where]
                if self.clear_pending[int(tell)]:
                    assert isinstance(clear, int), f"{self.step}: {name} touches the rings and left the pending clear behind"
                    assert np.array_equal(self.lib.arrays[clear], self.masks[int(tell)]), f"{self.step}: {name} sent other clears"
                    self.masks[int(tell)][:] = 0
                    self.clear_pending[int(tell)] = False
                    self.clears_sent[int(tell)] += 1
                else:
                    assert clear is None, f"{self.step}: {name} sent clears though none is pending"
            else:
                assert args[where] is None, f"{self.step}: {name} does not record and sent clears"
        return touches


class HostRunner(Runner):
    """The Runner, telling the model which rings a clear names."""

    def _clear_review(self, _=None) -> None:
        rooms = [self.rng.randrange(self.state.review_rooms) for _ in range(self.rng.randint(1, 2))]
        self.roster.clear_review(rooms)
        self.seen.cleared(self.label, False, rooms)

    def _clear_revtell(self, _=None) -> None:
        slots = [self.rng.randrange(self.state.cap) for _ in range(self.rng.randint(1, 3))]
        self.roster.clear_revtell(slots)
        self.seen.cleared(self.label, True, slots)


def host_blocks(rng: random.Random) -> list:
    """[an update, a call] for every kind after every single field alone, and after the pairs that share a mirror but not a
    flag; the clear blocks; random steps up to HOST_STEPS."""
    blocks = [[op_for(f), (kind, {})] for kind in KINDS for f in FIELDS]
    for pair in (("vis", "afk"), ("name", "igntell"), ("level", "afk"), ("muzzled", "igntell"), ("muzzle_level", "afk")):
        blocks += [[("update", pair), (kind, {})] for kind in KINDS]
    blocks += [[("update", apart(rng.sample(USER_FIELDS, n))), (kind, {})] for kind in KINDS for n in (2, 3, 6)]
    # afk and igntell alone, then a kind that reads the speaker mirror without them, then one that reads them: the mirror
    # is clean when the update comes, so only the flag of their own can bring it up
    blocks += [[("speak_many", {}), ("update", (f,)), (between, {}), (reader, {})] for f, readers in
               (("afk", ("tell_many", "look_many", "act_many")), ("igntell", ("tell_many",))) for between in ("speak_many", "input_many")
               for reader in readers]
    # the muzzle's two writers, one behind the other, and the kinds that read the bit behind each
    blocks += [[("update", (first,)), ("update", (second,)), (kind, {})] for first in MUZZLE_FIELDS for second in MUZZLE_FIELDS
               for kind in KINDS if "muzzled" in READS[kind]]
    # go_many's aftermath met first by every kind: a move with a dropped invite and a room returned to public
    blocks += [[("go_many", {"returns": True}), (kind, {})] for kind in KINDS]
    # ... and access_many's, which flips an access and drops an invite, and clone_many's, which besides moves the records
    # down; a set_many of whatever it draws
    blocks += [[(source, {"returns": True}), (kind, {})] for source in ("access_many", "clone_many") for kind in KINDS]
    blocks += [[("set_many", {}), (kind, {})] for kind in KINDS]
    # ... and act_many's: a move with a dropped invite and a room returned to public behind the look in its middle; a muzzle
    # set; whatever it draws
    blocks += [[("act_many", opts), (kind, {})] for opts in ({"returns": True}, {"muzzles": True}, {}) for kind in KINDS]
    # a .topic in the call or none, before every kind that reads the room table
    blocks += [[op_for("rooms.topic"), ("set_many", {"topic": topic}), (kind, {})] for topic in (True, False)
               for kind in KINDS if "rooms.topic" in READS[kind]]
    blocks += clear_blocks() * 3
    while sum(map(len, blocks)) < HOST_STEPS:
        blocks.append([random_op(rng)])
    rng.shuffle(blocks)
    return blocks


def host_run(lib, seed: int, ops=None, cap: int = 9, nclones: int = 4, review_rooms: int = REVIEW_ROOMS):
    rng = random.Random(seed)
    state = State(rng, cap, nclones, review_rooms)
    roster = new_roster(cap, nclones, review_rooms)
    state.seat(roster)
    host = Host(lib, roster, state)
    runner = HostRunner(rng, roster, state, "host", host, check=False, script=lib.script)
    if ops is None:                                                     # and a last round, so that whatever is stale is read
        ops = [op for b in host_blocks(rng) for op in b] + [(kind, {}) for kind in KINDS]
    for i, op in enumerate(ops):
        host.step = f"step {i} {op[0]}{list(op[1]) if len(op) > 1 and op[0] not in KINDS else ''}"
        runner.step(op)
        assert runner.bad == [], runner.bad
    return host, runner, ops


# ------------------------------------------------------------------ host tier
def test_the_field_tables_are_whole():
    assert set(FIELDS) == set(USER_FIELDS) | {f"rooms.{f}" for f in ROOM_FIELDS} | {f"clones.{f}" for f in CLONE_FIELDS} | {RELAY_NAMES}
    assert set(MIRROR_OF.values()) == set(MIRRORS) | {"names"} and len(KINDS) == 16 and set(READS) == set(KINDS)
    assert KINDS[7:10] == ("who_many", "rooms_many", "go_many")
    assert KINDS[10:14] == EVENT_KINDS == ("access_many", "clone_many", "set_many", "act_many") and len(EVENT_KINDS) == 4
    assert len(TABLE_KINDS) == 14 and len([(a, b) for a in TABLE_KINDS for b in TABLE_KINDS if a != b]) == 182
    assert set(TABLE_KINDS) == set(KINDS) - {"review_many", "revtell_many"}
    assert {f for f in FIELDS if MIRROR_OF[f] == "_speech"} >= {"prompt", "charmode_echo"} and {"prompt", "charmode_echo"} <= set(USER_FIELDS)
    assert MIRROR_OF["muzzle_level"] == MIRROR_OF["muzzled"] == "_speech" and set(MUZZLE_FIELDS) <= set(USER_FIELDS)
    assert {f for f in FIELDS if MIRROR_OF[f] == "_who"} == {"last_login", "away"}
    assert {f for f in FIELDS if MIRROR_OF[f] == "_go"} == {"in_phrase", "out_phrase", "invite_room"}
    assert MIRROR_OF["rooms.inlink"] == "_rooms" and {"_who", "_go"} <= set(MIRRORS)
    r = new_roster(3, 2)
    for m in MIRRORS:
        assert isinstance(getattr(r, m), np.ndarray), m
    for kind in KINDS:
        assert READS[kind] <= set(FIELDS) and UNREAD[kind] in set(FIELDS) - READS[kind], kind
        assert bool(READS[kind]) == (kind in TABLE_KINDS)
    # what the kernels read beyond what update()'s docstring and the issue's table say: tell_many reads the level
    assert "level" in READS["tell_many"] and "level" not in READS["speak_many"] and "command_mode" not in READS["tell_many"]
    assert READS["relay_many"] & {f"rooms.{f}" for f in ROOM_FIELDS} == set()
    # who_many prints of a room its name or its service; rooms_many reads of a slot whether it has a name; go_many reads a
    # clone record's owner and room, not what it hears; only rooms_many reads the inlink, only who_many the who row, only
    # go_many the go row
    assert READS["who_many"] & {f"rooms.{f}" for f in ROOM_FIELDS} == {"rooms.name", "rooms.netlink"}
    assert READS["rooms_many"] & set(USER_FIELDS) == set(TABLE_FIELDS) | {"name"}
    assert READS["go_many"] & {f"clones.{f}" for f in CLONE_FIELDS} == {"clones.owner", "clones.room"}
    assert READS["go_many"] & {f"rooms.{f}" for f in ROOM_FIELDS} == {"rooms.name", "rooms.access", "rooms.links", "rooms.netlink"}
    # access_many reads what go_many reads of the records, and of a room its name, access and links: get_room compares names
    # and reads nothing of a netlink, which the issue's table of this test left open; it does not read muzzled, which clone_many reads for a
    # .csay.  clone_many reads the owner and the room of a record and never what it hears, though the issue's table expected
    # all three fields; of a room the name and the access, not the links
    assert READS["access_many"] & {f"clones.{f}" for f in CLONE_FIELDS} == {"clones.owner", "clones.room"}
    assert READS["access_many"] & {f"rooms.{f}" for f in ROOM_FIELDS} == {"rooms.name", "rooms.access", "rooms.links"}
    assert READS["access_many"] & set(USER_FIELDS) == set(TABLE_FIELDS) | {"name", "vis", "level", "invite_room"}
    assert READS["clone_many"] & {f"clones.{f}" for f in CLONE_FIELDS} == {"clones.owner", "clones.room"}
    assert READS["clone_many"] & {f"rooms.{f}" for f in ROOM_FIELDS} == {"rooms.name", "rooms.access"}
    assert READS["clone_many"] & set(USER_FIELDS) == set(TABLE_FIELDS) | {"name", "vis", "level", "muzzled", "invite_room"}
    # set_many reads no record and no level, not muzzled and not the afk bit, which its kernel's argument comment lists;
    # the phrases, which go_many reads too; and of the room table the topic alone, in a call that holds a .topic
    assert READS["set_many"] & set(USER_FIELDS) == set(TABLE_FIELDS) | {"name", "vis", "command_mode", "igntell", "prompt", "charmode_echo",
                                                                      "afk_mesg", "desc", "in_phrase", "out_phrase"}
    assert READS["set_many"] - set(USER_FIELDS) == TOPIC_READS == {"rooms.topic"}
    # act_many reads what access_many reads of the records and of the go row, and of a room its name and its access: no links,
    # which the binding reads of the host mirror for its own deferral, and nothing of a netlink -- ACT_MOVE_AWAY is decided by
    # the target's room index --, both of which the issue's table of this test left open.  Of the speaker state the name, vis,
    # the level, the muzzled bit and the muzzle's level, and afk for a .wake: not igntell, command_mode or the set flags
    assert READS["act_many"] & set(USER_FIELDS) == set(TABLE_FIELDS) | {"name", "vis", "level", "muzzled", "muzzle_level", "afk",
                                                                      "invite_room"}
    assert READS["act_many"] & {f"clones.{f}" for f in CLONE_FIELDS} == {"clones.owner", "clones.room"}
    assert READS["act_many"] & {f"rooms.{f}" for f in ROOM_FIELDS} == {"rooms.name", "rooms.access"}
    assert not READS["act_many"] & {"clones.hear", "igntell", "command_mode", "in_phrase", "out_phrase", "rooms.topic", "rooms.desc",
                                    "rooms.links", "rooms.netlink", "prompt", "charmode_echo", "afk_mesg", "desc", RELAY_NAMES}
    assert reads_of("set_many", topic=True) == READS["set_many"] and reads_of("set_many") == READS["set_many"] - TOPIC_READS
    assert all(reads_of(kind, topic) == READS[kind] for kind in KINDS if kind != "set_many" for topic in (False, True))
    # the fields that exactly one kind reads, and which kind that is
    alone = {f: [k for k in KINDS if f in READS[k]] for f in FIELDS}
    assert {f: ks[0] for f, ks in alone.items() if len(ks) == 1} == {
        "rooms.inlink": "rooms_many", "last_login": "who_many", "away": "who_many", "prompt": "set_many", "charmode_echo": "set_many",
        "clones.hear": "relay_many", RELAY_NAMES: "relay_many", "rooms.desc": "look_many", "muzzle_level": "act_many"}
    assert alone["muzzled"] == ["speak_many", "input_many", "tell_many", "clone_many", "act_many"]
    # what the four newest kinds brought: the go row has more than one reader now
    assert alone["invite_room"] == ["go_many", "access_many", "clone_many", "act_many"] and alone["in_phrase"] == alone["out_phrase"] == ["go_many", "set_many"]
    assert all(ks for ks in alone.values())
    # the word of a quiet act_many names nobody: get_user looks for it, its first byte capitalised, inside every name
    rng = random.Random(1)
    drawn = {State.value(None, rng, "name", j) for j in range(1, 4000)} | {b"Guest0001", b"Mover0001"}
    assert not [name for name in drawn if NOWHERE.capitalize() in name or NOWHERE in name.lower()]


def test_no_call_kind_ever_reads_a_stale_field(fake):
    """On a roster with three ring rooms, where clone_many cannot record and passes every pending clear by."""
    the_safety_property(fake, REVIEW_ROOMS)


def test_no_call_kind_ever_reads_a_stale_field_with_a_ring_for_every_look_room(fake):
    """... and where clone_many(record=True) is a fifth kind that takes the pending review clear, after each source of one."""
    the_safety_property(fake, LOOK_ROOMS)


def the_safety_property(fake, review_rooms: int) -> None:
    host, runner, ops = host_run(fake, 20264, review_rooms=review_rooms)
    recording = RECORDING_KINDS + (("clone_many",) if review_rooms == LOOK_ROOMS else ())
    assert len(ops) >= HOST_STEPS and runner.steps == len(ops)
    assert all(n >= 20 for n in host.runs["host"].values()), host.runs
    # every kind was called with every field stale: those it reads (and was passed, or the run had stopped above) ...
    missing = [(k, f) for k in KINDS for f in FIELDS if (k, f) not in host.stale_at_call]
    assert missing == []
    # ... and those it does not read, which a kind that reads them found clean later
    unread = {(k, f) for k in KINDS for f in FIELDS if f not in READS[k]}
    assert unread <= host.awaiting and unread <= host.read_clean_later, sorted(unread - host.read_clean_later)[:5]
    # a clear went down with each of the kinds that can carry it, and each kind was the first after a clear
    assert host.clears_sent[0] >= 15 and host.clears_sent[1] >= 6
    assert set(host.first_after_clear_review) == set(recording) | {"review_many"}
    assert set(host.first_after_clear_revtell) == {"tell_many", "revtell_many"}
    # ... a clear that a go_many, an access_many, a clone_many or an act_many left behind included, after each of the four
    # sources
    for source, first in host.first_after.items():
        assert set(first) == set(recording) | {"review_many"}, (source, first)
    c = runner.counts
    # the blocks alone hold 34 go_many calls that move, drop an invite and return a room: one per kind, six clear blocks
    # thrice; as many access_many calls that set a room public, as many clone_many calls whose .destroy returns one, and as
    # many act_many calls that move a user out of a room which returns, with two invitations cleared each
    assert c["moves"] >= 33 and c["returned_public"] >= 33 and c["invites_dropped"] >= 33 and c["deferred"] > 0, c
    assert c["access_returned"] >= 33 and c["destroy_returned"] >= 33 and c["destroyed"] >= 33 and c["compacted"] > 0, c
    assert c["act_returned"] >= 33 and c["act_moved"] >= 33 and c["act_invites_cleared"] >= 66 and c["act_muzzled"] >= 16, c
    assert all(c[name] > 0 for name in EVENT_COUNTS if name != "said_recorded"), c
    assert (c["said_recorded"] >= 18) == (review_rooms == LOOK_ROOMS) and (c["said_recorded"] > 0) == (review_rooms == LOOK_ROOMS), c
    for kind in KINDS:
        for f in READS[kind]:
            assert host.after_read.get(f"{kind}/{f}", 0) > 0, (kind, f)
        assert host.after_unread.get(kind, 0) > 0, kind


@pytest.mark.parametrize("ops", [
    # afk lives in the speaker mirror's flags byte with a flag of its own: a speak_many in between must not lose it
    [("tell_many", {}), ("update", ("afk",)), ("speak_many", {}), ("look_many", {})],
    [("look_many", {}), ("update", ("igntell",)), ("input_many", {}), ("tell_many", {})],
    # ... and with a field of the other flag in the same update, whichever kind uploads the mirror cleans both
    [("update", ("vis", "afk")), ("speak_many", {}), ("tell_many", {}), ("update", ("afk",)), ("look_many", {}), ("tell_many", {})],
    [("update", ("name", "igntell")), ("tell_many", {}), ("speak_many", {}), ("look_many", {})],
    # a name set between two relay_many calls, with a look_many that uploads the room table in between
    [("relay_many", {}), ("set_rooms", ("name",)), ("look_many", {}), ("relay_many", {}), ("relay_many", {})],
    # a clear waits for a call that touches its rings: the calls that do not record leave it pending
    [("clear_review",), ("plan_many", {"record": False}), ("speak_many", {"record": False}), ("tell_many", {"record": True}),
     ("relay_many", {"record": True}), ("review_many", {})],
    [("clear_revtell",), ("tell_many", {"record": False}), ("review_many", {}), ("revtell_many", {}), ("tell_many", {"record": True})],
    # afk alone passes by rooms_many and go_many, which do not read it, and reaches each kind that does
    [("tell_many", {}), ("update", ("afk",)), ("rooms_many", {}), ("go_many", {"quiet": True}), ("who_many", {}), ("update", ("afk",)),
     ("go_many", {}), ("rooms_many", {}), ("look_many", {}), ("update", ("afk",)), ("rooms_many", {}), ("go_many", {}), ("tell_many", {})],
    # vis and afk in one update: go_many or rooms_many uploads the mirror and cleans both
    [("tell_many", {}), ("update", ("vis", "afk")), ("go_many", {}), ("tell_many", {}), ("update", ("vis", "afk")), ("rooms_many", {}),
     ("look_many", {}), ("who_many", {})],
    # a go_many that moves, drops an invite and returns a room to public, met first by each other table-reading kind
    [op for kind in TABLE_KINDS if kind != "go_many" for op in (("go_many", {"returns": True}), (kind, {}), ("go_many", {}))],
    # ... the room table it left dirty taken by who_many or rooms_many, or by nobody, before the next go_many
    [("go_many", {"returns": True}), ("who_many", {}), ("go_many", {}), ("go_many", {"returns": True}), ("rooms_many", {}), ("go_many", {}),
     ("go_many", {"returns": True}), ("plan_many", {}), ("go_many", {}), ("look_many", {})],
    # the who table between two who_many calls, with a look_many in between: only who_many cleans it
    [("who_many", {}), ("update", ("last_login",)), ("look_many", {}), ("who_many", {}), ("update", ("away",)), ("look_many", {}),
     ("rooms_many", {}), ("who_many", {})],
    # the clear a go_many leaves waits like clear_review's
    [("go_many", {"returns": True}), ("plan_many", {"record": False}), ("who_many", {}), ("go_many", {}), ("tell_many", {"record": True}),
     ("speak_many", {"record": True}), ("review_many", {})],
    # the three examples no test noticed: a tell_many behind a set_many that may toggle igntell, a relay_many behind a
    # clone_many that destroyed record 0, a look_many behind a set_many without a .topic that met a dirty room table
    [("tell_many", {}), ("set_many", {}), ("tell_many", {}), ("set_many", {}), ("set_many", {}), ("tell_many", {}), ("look_many", {}),
     ("who_many", {})],
    [("relay_many", {}), ("clone_many", {"returns": True}), ("relay_many", {}), ("go_many", {}), ("clone_many", {}), ("relay_many", {}),
     ("access_many", {})],
    [("look_many", {}), ("set_rooms", ("topic",)), ("set_many", {"topic": False}), ("look_many", {}), ("set_rooms", ("topic",)),
     ("set_many", {"topic": True}), ("look_many", {}), ("rooms_many", {})],
    # an access_many that returns a room to public, met first by each other table-reading kind, as go_many's above
    [op for kind in TABLE_KINDS if kind != "access_many" for op in (("access_many", {"returns": True}), (kind, {}), ("access_many", {}))],
    # ... and a clone_many whose .destroy returns one and moves the records down
    [op for kind in TABLE_KINDS if kind != "clone_many" for op in (("clone_many", {"returns": True}), (kind, {}), ("clone_many", {}))],
    # the clear an access_many leaves waits past the calls that do not record, access_many itself among them
    [("access_many", {"returns": True}), ("plan_many", {"record": False}), ("who_many", {}), ("access_many", {"quiet": True}),
     ("clone_many", {"record": True}), ("set_many", {}), ("speak_many", {"record": True}), ("review_many", {})],
    # every set_many kind of call between two calls of every kind that reads what it may set
    [op for kind in TABLE_KINDS for op in (("set_many", {"topic": None if kind == "set_many" else kind in ("look_many", "rooms_many")}),
                                           (kind, {}))],
    # afk alone passes by rooms_many and a quiet go_many, and act_many, whose .wake reads it, takes it; after the next update
    # of afk an act_many, and the kinds that read afk behind it find nothing stale
    [("tell_many", {}), ("update", ("afk",)), ("rooms_many", {}), ("go_many", {"quiet": True}), ("act_many", {}), ("update", ("afk",)),
     ("act_many", {}), ("tell_many", {}), ("look_many", {}), ("who_many", {})],
    # vis and afk in one update: act_many uploads the mirror and cleans both flags outright
    [("tell_many", {}), ("update", ("vis", "afk")), ("act_many", {}), ("tell_many", {}), ("set_many", {}), ("look_many", {})],
    # an act_many that moves a user, clears two invitations and returns a room to public behind the look in its middle, met
    # first by each other table-reading kind
    [op for kind in TABLE_KINDS if kind != "act_many" for op in (("act_many", {"returns": True}), (kind, {}), ("act_many", {}))],
    # ... and one that muzzles, by each kind that reads the muzzled bit on the device
    [op for kind in ("speak_many", "input_many", "tell_many", "clone_many", "act_many") for op in (("act_many", {"muzzles": True}), (kind, {}))],
    # the clear an act_many leaves waits past the calls that do not record, act_many itself among them
    [("act_many", {"returns": True}), ("plan_many", {"record": False}), ("who_many", {}), ("act_many", {"quiet": True}),
     ("clone_many", {"record": True}), ("set_many", {}), ("speak_many", {"record": True}), ("review_many", {})],
    # the muzzle's two writers: the level, then the bit alone twice, an act_many behind each; and the bit taken and put back
    # under a GOD's level, which a WIZ may not remove
    [("update", ("muzzle_level",)), ("act_many", {}), ("update", ("muzzled",)), ("act_many", {}), ("update", ("muzzled",)), ("act_many", {}),
     ("act_many", {"above": True}), ("speak_many", {}), ("act_many", {})],
], ids=["afk-speak-look", "igntell-input-tell", "vis+afk", "name+igntell", "names-between-relays", "review-clear-waits",
        "revtell-clear-waits", "afk-rooms-go", "vis+afk-go-rooms", "go-moves-then-each", "go-returns-rooms-table", "who-table",
        "go-clear-waits", "set-then-tell", "destroy-then-relay", "topicless-set-then-look", "access-returns-then-each",
        "destroy-returns-then-each", "access-clear-waits", "set-then-each", "afk-then-wake", "vis+afk-act", "act-moves-then-each",
        "act-muzzles-then-each", "act-clear-waits", "bit-then-level"])
def test_the_rules_that_are_not_uniform_one_by_one(fake, ops):
    host, runner, _ = host_run(fake, 5, ops=ops)
    assert runner.steps == len(ops)


QUIET, RETURNS = ("go_many", {"quiet": True}), ("go_many", {"returns": True})
#: an act_many that moves slot 1 and returns the room it left: a look in its middle, as in the go_many that moves
ACT_RETURNS = ("act_many", {"returns": True})


def was_passed(host, ops) -> list:
    """Per op that is a call, the mirrors its library call was passed; the look inside a go_many or an act_many that moved
    is left out."""
    log, out = list(host.log), []
    for op in ops:
        if op[0] in KINDS:
            kind, passed = log.pop(0)
            assert kind == op[0]
            out.append(passed)
            if op in (RETURNS, ACT_RETURNS):
                assert log.pop(0)[0] == "look_many"
        else:
            out.append(None)
    assert not log
    return out


@pytest.mark.parametrize("reader", ["who_many", "look_many", "tell_many"])
def test_afk_alone_passes_by_the_kinds_that_do_not_read_it(fake, reader):
    """afk updated alone, then rooms_many and go_many: neither reads it, neither is passed the speaker mirror for it, and
    neither may lose ``_private_dirty``: the first kind that reads afk still gets the mirror."""
    ops = [("tell_many", {}), ("who_many", {}), QUIET, ("update", ("afk",)), ("rooms_many", {}), QUIET, (reader, {}), (reader, {})]
    host, _, _ = host_run(fake, 5, ops=ops)
    passed = was_passed(host, ops)
    assert "_speech" not in passed[4] and "_speech" not in passed[5] and "_speech" in passed[6] and "_speech" not in passed[7]


@pytest.mark.parametrize("uploader", ["rooms_many", "go_many"])
def test_vis_and_afk_in_one_update_go_up_together(fake, uploader):
    """vis dirties the speaker mirror for everybody: rooms_many or go_many uploads it whole and cleans afk with it."""
    ops = [("tell_many", {}), ("who_many", {}), QUIET, ("update", ("vis", "afk")), (uploader, {"quiet": True}), ("tell_many", {}),
           ("look_many", {})]
    host, _, _ = host_run(fake, 5, ops=ops)
    passed = was_passed(host, ops)
    assert "_speech" in passed[4] and "_speech" not in passed[5] and "_speech" not in passed[6]
    assert not host.roster._private_dirty


@pytest.mark.parametrize("kind", [k for k in TABLE_KINDS if k != "go_many"])
def test_a_go_many_that_moves_leaves_the_table_clean_and_its_own_tables_dirty(fake, kind):
    """The look inside the go call uploaded the table, so the next kind is passed none.  The move dropped an invite and
    returned a room to public: the next go_many is passed the go table, and the room table unless a kind in between took it.
    Of the four kinds that keep go_many's tables, a call that changes nothing: access_many, clone_many and act_many take both,
    a set_many without a ``.topic`` takes the go table and leaves the room table behind."""
    ops = [(k, {}) for k in TABLE_KINDS if k != "go_many"] + [QUIET, RETURNS, (kind, {"quiet": True} if kind in EVENT_KINDS else {}),
                                                                QUIET, QUIET]
    host, runner, _ = host_run(fake, 5, ops=ops)
    passed = was_passed(host, ops)
    moved, nxt, later, last = passed[-4:]
    assert runner.counts["moves"] == 1 and runner.counts["invites_dropped"] >= 1 and runner.counts["returned_public"] == 1
    assert "_table" not in nxt and "_table" not in later
    assert ("_rooms" in nxt) == (kind in ("look_many", "who_many", "rooms_many", "access_many", "clone_many", "act_many"))   # the room table has one flag
    assert ("_go" in nxt) == (kind in EVENT_KINDS)
    assert ("_go" in later) == ("_go" not in nxt) and ("_rooms" in later) == ("_rooms" not in nxt)
    assert last == frozenset()


def test_only_who_many_cleans_the_who_table(fake):
    ops = [("who_many", {}), ("look_many", {}), ("update", ("last_login",)), ("look_many", {}), ("who_many", {}), ("who_many", {})]
    host, _, _ = host_run(fake, 5, ops=ops)
    passed = was_passed(host, ops)
    assert "_who" in passed[0] and "_who" not in passed[3] and host.roster._who_dirty is False
    assert "_who" in passed[4] and "_who" not in passed[5]


def quietly(kind: str) -> tuple:
    """A call of ``kind`` that changes nothing on the roster: the kinds that can are asked not to."""
    return (kind, {"quiet": True, "topic": False, "record": False})


#: a call of every table-reading kind that changes nothing, set_many last: every mirror is up and every flag down
WARM = [quietly(kind) for kind in TABLE_KINDS if kind != "set_many"] + [("set_many", {"quiet": True, "topic": True})]
#: the kinds whose calls upload the speaker mirror after an update of name, vis, muzzled, command_mode or level
SPEAKER_KINDS = tuple(kind for kind in TABLE_KINDS if "name" in READS[kind])


#: a seed whose State has all four clone records owned: when record 0 is destroyed, record 1 moves down into its place, and
#: the Runner has no record 0 to make anew -- its own set_clones would mark the records as the apply step should have
DENSE_RECORDS = 6


def after_warming(fake, ops, seed: int = 5):
    """WARM, then ``ops``: the run's host and runner, and what each op of ``ops`` was passed."""
    host, runner, _ = host_run(fake, seed, ops=WARM + ops)
    return host, runner, was_passed(host, WARM + ops)[len(WARM):]


@pytest.mark.parametrize("field", ["prompt", "charmode_echo"])
def test_prompt_and_charmode_echo_alone_wait_for_set_many(fake, field):
    """Updated alone, they raise ``_set_dirty`` and nothing else: every other kind passes by without the speaker mirror and
    without losing the flag, the next set_many gets the mirror, and its repeat does not."""
    others = [quietly(kind) for kind in TABLE_KINDS if kind != "set_many"]
    host, _, passed = after_warming(fake, [("update", (field,))] + others + [quietly("set_many"), quietly("set_many")])
    assert SPEAKER_KINDS == ("speak_many", "input_many", "tell_many", "look_many", "who_many", "rooms_many", "go_many", "access_many",
                             "clone_many", "set_many", "act_many")
    for (kind, _), got in zip(others, passed[1:-2]):
        assert "_speech" not in got, kind
    assert "_speech" in passed[-2] and "_speech" not in passed[-1] and not host.roster._set_dirty


@pytest.mark.parametrize("uploader", [kind for kind in SPEAKER_KINDS if kind != "set_many"])
def test_vis_and_prompt_in_one_update_go_up_with_whoever_uploads_the_speaker_mirror(fake, uploader):
    """vis dirties the speaker mirror for everybody: the kind that uploads it brings prompt up with it, so the set_many
    behind it reads nothing stale whether or not it is passed the mirror again; its repeat is passed none."""
    host, _, passed = after_warming(fake, [("update", ("vis", "prompt")), quietly(uploader), quietly("set_many"), quietly("set_many")])
    assert "_speech" in passed[1] and "_speech" not in passed[3]
    assert not (host.roster._speech_dirty or host.roster._set_dirty or host.roster._private_dirty)


@pytest.mark.parametrize("field", ["afk", "igntell"])
def test_afk_and_igntell_alone_go_up_with_set_many(fake, field):
    """set_many reads igntell and not afk, and uploads the speaker mirror on ``_private_dirty`` either way, clearing it: the
    tell_many and the look_many behind it read neither stale and are not passed the mirror again."""
    host, _, passed = after_warming(fake, [("update", (field,)), quietly("set_many"), ("tell_many", {}), ("look_many", {})])
    assert "_speech" in passed[1] and "_speech" not in passed[2] and "_speech" not in passed[3]
    assert not host.roster._private_dirty


def test_a_set_many_without_a_topic_keeps_the_room_table_back(fake):
    """After ``set_rooms(topic=)`` a set_many that holds no ``.topic`` is not passed the room table and leaves it dirty: the
    look_many behind it gets it.  With a ``.topic`` in the call it is passed, and look_many gets none."""
    host, runner, passed = after_warming(fake, [("set_rooms", ("topic",)), quietly("set_many"), ("look_many", {}),
                                                ("set_rooms", ("topic",)), ("set_many", {"quiet": True, "topic": True}), ("look_many", {})])
    assert "_rooms" not in passed[1] and "_rooms" in passed[2]
    assert "_rooms" in passed[4] and "_rooms" not in passed[5]
    assert runner.counts["topicless_dirty"] == 1 and runner.counts["topic_calls"] == 2      # WARM's, and this one


@pytest.mark.parametrize("source", ["access_many", "clone_many"])
def test_access_many_and_clone_many_clean_the_room_table_for_the_others(fake, source):
    followers = [("look_many", {}), ("who_many", {}), ("rooms_many", {}), QUIET]
    _, _, passed = after_warming(fake, [("set_rooms", ("access",)), quietly(source)] + followers)
    assert "_rooms" in passed[1] and all("_rooms" not in got for got in passed[2:])


def test_an_invitation_dirties_the_go_table_for_go_many(fake):
    host, runner, passed = after_warming(fake, [("access_many", {"invites": True}), QUIET, QUIET])
    assert runner.counts["access_effective"] == 1 and runner.state.users[1]["invite"] == runner.state.users[0]["room"]
    # the Runner's own updates before the call went up with it; what the go_many gets, the call's apply step left
    assert {"_go", "_rooms", "_speech", "_table"} <= passed[0] and passed[1] == {"_go"} and passed[2] == frozenset()


def test_the_clear_an_access_many_leaves_goes_down_with_the_first_recording_call(fake):
    ops = [("access_many", {"returns": True}), ("plan_many", {"record": False}), ("who_many", {}), quietly("access_many"),
           ("speak_many", {"record": True}), ("review_many", {})]
    host, runner, _ = after_warming(fake, ops)
    assert runner.counts["access_returned"] == 1 and host.clears_sent == [1, 0] and not host.clear_pending[0]
    assert host.first_after["access"] == {"speak_many": 1} and host.first_after_clear_review == {"speak_many": 1}


@pytest.mark.parametrize("follower", [("relay_many", {}), QUIET, quietly("access_many")], ids=["relay_many", "go_many", "access_many"])
def test_a_destroy_that_compacts_gives_each_follower_the_clone_records_once(fake, follower):
    """The records behind the destroyed one moved down in the mirrors, in place: the index that a relay_many or a go_many
    saw before the call means another record after it, and each kind that reads them is passed them, once."""
    host, runner, passed = after_warming(fake, [("clone_many", {"returns": True}), follower, follower], seed=DENSE_RECORDS)
    assert all(r[0] is not None for r in runner.state.records[:3]) and runner.state.records[3][0] is None
    assert runner.counts["destroyed"] == 1 and runner.counts["compacted"] == 1 and runner.counts["destroy_returned"] == 1
    assert "_clones" in passed[1] and "_clones" not in passed[2]
    assert ("_rooms" in passed[1]) == (follower[0] != "relay_many") and "_rooms" not in passed[2]


def test_the_binding_refuses_a_recording_clone_many_without_a_ring_for_every_look_room(fake):
    """Why the Runner drops ``record`` on the rosters with three ring rooms."""
    host, runner, _ = host_run(fake, 5, ops=WARM)
    actor = runner.state.speakers()[0]
    with pytest.raises(ValueError, match="record: a clone may speak in any of the 5 look rooms"):
        runner.roster.clone_many([(actor, device.COM_CSAY, b"x y", 3)], max_clones=1, gatecrash_level=0, min_private_users=0, record=True)
    assert fake.calls == [] and fake.script == []


def test_the_model_notices_a_mirror_that_is_not_passed(fake, monkeypatch):
    """The safety property is not vacuous: a look_many that forgets the afk flag's own dirty flag is caught."""
    real = device.Roster.look_many

    def forgetful(self, slots):
        keep, self._private_dirty = self._private_dirty, False
        try:
            return real(self, slots)
        finally:
            self._private_dirty = self._private_dirty or keep
    monkeypatch.setattr(device.Roster, "look_many", forgetful)
    with pytest.raises(AssertionError, match=r"look_many \(nd_roster_look\) read \['afk'\] stale"):
        host_run(fake, 5, ops=[("speak_many", {}), ("update", ("afk",)), ("look_many", {})])


GO_SUBSETS = ["+".join(t for b, t in enumerate(GO_TABLES) if i >> b & 1) for i in range(16)]
#: set_many's: every subset of its first four kept tables, with the room table clean, passed, or dirty and kept back
SET_SUBSETS = ["+".join([t for b, t in enumerate(SET_TABLES[:4]) if i >> b & 1] + rooms) for i in range(16)
               for rooms in ([], [SET_TABLES[4]], [KEPT_BACK])]


def assert_the_counts(c: dict, device: bool) -> None:
    """What a seed's run counts of the four newest kinds, from the model's calls.  The floors are those of a run of the
    child's streams over the library that computes nothing (the dry run below asserts them too), rounded down."""
    print(c)
    assert c["moves"] >= MOVES and c["returned_public"] >= RETURNED and c["deferred"] >= DEFERRED, c
    assert c["invites_dropped"] >= RETURNED and c["who_lines"] >= WHO_LINES and c["rooms_listings"] >= ROOMS_LISTINGS, c
    assert set(EVENT_FLOORS) == set(EVENT_COUNTS) and all(floor > 0 for floor in EVENT_FLOORS.values())
    short = {name: (c[name], floor) for name, floor in EVENT_FLOORS.items() if c[name] < floor}
    assert not short, short


def assert_the_coverage(cov: dict) -> None:
    assert len(cov["runs"]) == 2 * (len(CAPACITIES) + 1)
    for label, runs in cov["runs"].items():
        assert set(runs) == set(KINDS) and all(n >= 8 for n in runs.values()), (label, runs)
    for kind in KINDS:
        for f in READS[kind]:
            assert cov["after_read"].get(f"{kind}/{f}", 0) > 0, (kind, f)
        assert cov["after_unread"].get(kind, 0) > 0, kind
    for kind in RECORDING_KINDS:
        assert cov["first_after_clear_review"].get(kind, 0) > 0, kind
    for kind in ("tell_many", "revtell_many"):
        assert cov["first_after_clear_revtell"].get(kind, 0) > 0, kind
    # the clear that a go_many, an access_many, a clone_many or an act_many left behind; clone_many is the first to touch the
    # rings only on the 130-slot roster of each seed, which has a ring for every look room.  An act_many returns no room on
    # the roster of one slot, which has nobody to move: what is asserted of its clears holds over the union of the rosters
    assert cov["first_after_clear_review"].get("clone_many", 0) > 0
    for source in ("go", "access", "clone", "act"):
        for kind in RECORDING_KINDS + ("clone_many", "review_many"):
            assert cov[f"first_after_{source}_clear"].get(kind, 0) > 0, (source, kind)
    for table, want in (("go", GO_SUBSETS), ("access", GO_SUBSETS), ("clone", GO_SUBSETS), ("act", GO_SUBSETS), ("set", SET_SUBSETS)):
        seen = cov[f"{table}_subsets"]
        assert sorted(seen) == sorted(want) and all(n > 0 for n in seen.values()), (table, sorted(set(want) ^ set(seen)))


def forgetting(monkeypatch, method: str, flag: str) -> None:
    """``Roster.method``, from its second call on, with ``flag`` down while it runs, and as it was, or as the call set it,
    afterwards."""
    real = getattr(device.Roster, method)
    calls = []

    def forgetful(self, *args, **kw):
        calls.append(1)
        if len(calls) == 1:
            return real(self, *args, **kw)
        keep = getattr(self, flag)
        setattr(self, flag, False)
        try:
            return real(self, *args, **kw)
        finally:
            setattr(self, flag, getattr(self, flag) or keep)
    monkeypatch.setattr(device.Roster, method, forgetful)


def test_the_model_notices_a_go_many_that_forgets_the_go_table(fake, monkeypatch):
    forgetting(monkeypatch, "go_many", "_go_dirty")
    with pytest.raises(AssertionError, match=r"go_many \(nd_roster_go\) read \['invite_room'\] stale"):
        host_run(fake, 5, ops=[QUIET, ("update", ("invite_room",)), ("go_many", {})])


def test_the_model_notices_a_who_many_that_forgets_the_who_table(fake, monkeypatch):
    forgetting(monkeypatch, "who_many", "_who_dirty")
    with pytest.raises(AssertionError, match=r"who_many \(nd_roster_who\) read \['last_login'\] stale"):
        host_run(fake, 5, ops=[("who_many", {}), ("update", ("last_login",)), ("who_many", {})])


def test_the_model_notices_a_move_that_does_not_mark_the_table(fake, monkeypatch):
    """go_many's apply step moves the movers through ``update``: were the table not marked dirty there, the look inside the
    call would read the table as it was before the move."""
    real_go, real_update = device.Roster.go_many, device.Roster.update
    applying = []

    def go_many(self, *args, **kw):
        applying.append(True)
        try:
            return real_go(self, *args, **kw)
        finally:
            applying.pop()

    def update(self, *args, **kw):
        keep = self._dirty
        real_update(self, *args, **kw)
        if applying:
            self._dirty = keep
    monkeypatch.setattr(device.Roster, "go_many", go_many)
    monkeypatch.setattr(device.Roster, "update", update)
    with pytest.raises(AssertionError, match=r"look_many \(nd_roster_look\) read \['colour', 'ignall', 'ignshout', 'login', 'room'\] stale"):
        host_run(fake, 5, ops=[QUIET, RETURNS])


def test_the_model_notices_a_set_many_that_forgets_its_own_flag(fake, monkeypatch):
    forgetting(monkeypatch, "set_many", "_set_dirty")
    with pytest.raises(AssertionError, match=r"set_many \(nd_roster_set\) read \['prompt'\] stale"):
        host_run(fake, 5, ops=[quietly("set_many"), ("update", ("prompt",)), quietly("set_many")])


def test_the_model_notices_a_set_many_with_a_topic_that_forgets_the_room_table(fake, monkeypatch):
    forgetting(monkeypatch, "set_many", "_rooms_dirty")
    topic = ("set_many", {"quiet": True, "topic": True})
    with pytest.raises(AssertionError, match=r"set_many \(nd_roster_set\) read \['rooms.topic'\] stale"):
        host_run(fake, 5, ops=[topic, ("set_rooms", ("topic",)), topic])


def unmarked_while_applying(monkeypatch, call: str, through: str, flag: str) -> None:
    """``Roster.call`` whose apply step goes through ``Roster.through`` without raising ``flag``."""
    real_call, real_through = getattr(device.Roster, call), getattr(device.Roster, through)
    applying = []

    def calling(self, *args, **kw):
        applying.append(True)
        try:
            return real_call(self, *args, **kw)
        finally:
            applying.pop()

    def passing(self, *args, **kw):
        keep = getattr(self, flag)
        real_through(self, *args, **kw)
        if applying:
            setattr(self, flag, keep)
    monkeypatch.setattr(device.Roster, call, calling)
    monkeypatch.setattr(device.Roster, through, passing)


def test_the_model_notices_an_invitation_that_does_not_mark_the_go_table(fake, monkeypatch):
    unmarked_while_applying(monkeypatch, "access_many", "update", "_go_dirty")
    with pytest.raises(AssertionError, match=r"go_many \(nd_roster_go\) read \['invite_room'\] stale"):
        host_run(fake, 5, ops=[QUIET, ("access_many", {"invites": True}), QUIET])


def test_the_model_notices_a_destroy_that_does_not_mark_the_records(fake, monkeypatch):
    unmarked_while_applying(monkeypatch, "clone_many", "set_clones", "_clones_dirty")
    with pytest.raises(AssertionError, match=r"relay_many \(nd_roster_relay\w*\) read \['clones\.\w+'[^\]]*\] stale"):
        host_run(fake, DENSE_RECORDS, ops=[quietly("clone_many"), ("clone_many", {"returns": True}), ("relay_many", {})])


def test_the_model_notices_a_set_many_that_cleans_the_room_table_without_a_topic(fake, monkeypatch):
    real = device.Roster.set_many

    def eager(self, events):
        try:
            return real(self, events)
        finally:
            self._rooms_dirty = False
    monkeypatch.setattr(device.Roster, "set_many", eager)
    with pytest.raises(AssertionError, match=r"look_many \(nd_roster_look\) read \['rooms.topic'\] stale"):
        host_run(fake, 5, ops=[("look_many", {}), ("set_rooms", ("topic",)), quietly("set_many"), ("look_many", {})])


def test_afk_alone_goes_up_with_act_many_and_is_clean_for_the_kinds_behind_it(fake):
    """``.wake`` reads the target's afk bit: act_many is passed the speaker mirror on ``_private_dirty`` alone, which rooms_many
    and go_many pass by, and clears the flag outright; tell_many, look_many and who_many behind it are passed none."""
    ops = [("update", ("afk",)), quietly("rooms_many"), QUIET, quietly("act_many"), ("tell_many", {}), ("look_many", {}), ("who_many", {}),
           quietly("act_many")]
    host, runner, passed = after_warming(fake, ops)
    assert "_speech" not in passed[1] and "_speech" not in passed[2] and "_speech" in passed[3]
    assert all("_speech" not in got for got in passed[4:])
    assert runner.counts["act_private_alone"] == 1 and not host.roster._private_dirty


def test_an_act_many_that_moves_looks_in_the_middle_and_leaves_its_own_tables_dirty(fake):
    """The look inside the call uploaded the moved table; the room returned to public and the invitations cleared behind
    that look leave the room table and the go table for the next kind that keeps them, once."""
    host, runner, passed = after_warming(fake, [ACT_RETURNS, QUIET, QUIET])
    c = runner.counts
    assert (c["act_moved"], c["act_returned"], c["act_invites_cleared"], c["act_effective"]) == (1, 1, 2, 1)
    assert {"_table", "_speech", "_rooms", "_go"} <= passed[0] and passed[1] == {"_rooms", "_go"} and passed[2] == frozenset()
    assert host.clear_pending[0] and host.clear_from["host"] == "act"


def test_an_act_many_that_muzzles_gives_the_next_reader_the_speaker_mirror_once(fake):
    host, runner, passed = after_warming(fake, [("act_many", {"muzzles": True}), ("speak_many", {}), ("speak_many", {})])
    assert runner.counts["act_muzzled"] == 1 and runner.state.users[1]["muzzle"] == device.MAX_LEVEL
    assert int(host.roster._speech[1, 15]) == device.MAX_LEVEL and host.roster._speech[1, device.USER_NAME_LEN + 1] & 2
    assert "_speech" in passed[1] and "_speech" not in passed[2]


def test_a_muzzle_whose_bit_was_taken_and_put_back_keeps_its_level(fake):
    """``update(muzzle_level=GOD)``, ``update(muzzled=0)``, ``update(muzzled=1)``: byte 15 still says GOD, and the model
    answers a WIZ's ``.unmuzzle`` with ACT_UNMUZZLE_ABOVE; nothing changed, so the speak_many behind it is passed nothing."""
    host, runner, passed = after_warming(fake, [("act_many", {"above": True}), ("speak_many", {}), quietly("act_many")])
    u = runner.state.users[1]
    assert (u["muzzled"], u["muzzle"]) == (1, device.MAX_LEVEL) and runner.state.users[0]["level"] == 2
    assert int(host.roster._speech[1, 15]) == device.MAX_LEVEL and host.roster._speech[1, device.USER_NAME_LEN + 1] & 2
    assert runner.counts["act_unmuzzle_above"] == 1 and runner.counts["act_effective"] == 0
    assert "_speech" in passed[0] and "_speech" not in passed[1] and passed[2] == frozenset()


def test_the_binding_refuses_muzzled_and_muzzle_level_in_one_update(fake):
    """Why ``random_op`` and ``Runner._update`` never draw both."""
    host, runner, _ = host_run(fake, 5, ops=[("update", ("muzzled", "afk", "muzzle_level")), ("update", ("muzzle_level", "muzzled"))])
    assert apart(("muzzled", "afk", "muzzle_level")) == ("muzzled", "afk") and apart(("muzzle_level", "muzzled")) == ("muzzle_level",)
    assert all(len(set(op[1]) & set(MUZZLE_FIELDS)) < 2 for op in (random_op(random.Random(i)) for i in range(3000)) if op[0] == "update")
    with pytest.raises(ValueError, match="muzzled and muzzle_level cannot be given in one update"):
        runner.roster.update(0, muzzled=1, muzzle_level=2)


def test_the_model_notices_an_act_many_that_ignores_the_private_flag(fake, monkeypatch):
    """act_many's upload rule is its own: were it go_many's, a ``.wake`` would read the afk bit of before the update."""
    forgetting(monkeypatch, "act_many", "_private_dirty")
    with pytest.raises(AssertionError, match=r"act_many \(nd_roster_act\) read \['afk'\] stale"):
        host_run(fake, 5, ops=[quietly("act_many"), ("update", ("afk",)), quietly("act_many")])


def test_the_model_notices_a_muzzle_that_does_not_mark_the_speaker_mirror(fake, monkeypatch):
    unmarked_while_applying(monkeypatch, "act_many", "update", "_speech_dirty")
    with pytest.raises(AssertionError, match=r"speak_many \(nd_roster_speak\) read \['muzzled'\] stale"):
        host_run(fake, 5, ops=[quietly("act_many"), ("act_many", {"muzzles": True}), ("speak_many", {})])


def test_the_model_notices_an_act_many_whose_move_does_not_mark_the_table(fake, monkeypatch):
    """The look in the middle of the apply step would read the table as it was before the move."""
    unmarked_while_applying(monkeypatch, "act_many", "update", "_dirty")
    with pytest.raises(AssertionError, match=r"look_many \(nd_roster_look\) read \['colour', 'ignall', 'ignshout', 'login', 'room'\] stale"):
        host_run(fake, 5, ops=[quietly("act_many"), ACT_RETURNS])


@pytest.mark.parametrize("follower", ["look_many", "rooms_many"])
def test_the_model_notices_an_act_many_that_returns_a_room_without_marking_the_room_table(fake, monkeypatch, follower):
    unmarked_while_applying(monkeypatch, "act_many", "set_rooms", "_rooms_dirty")
    with pytest.raises(AssertionError, match=rf"{follower} \(nd_roster_\w+\) read \['rooms.access'\] stale"):
        host_run(fake, 5, ops=[quietly("act_many"), ACT_RETURNS, (follower, {})])


def test_the_device_stream_alone_reaches_what_the_device_tier_asserts(fake):
    """The child's own streams, with its seeds, over the library that computes nothing: the counts that the GPU tier asserts
    besides ``n_bad == 0`` come from the model's calls, so the floors are known to be reached before a device is asked."""
    class Dry(Coverage):
        def called(self, *args, **kw):
            super().called(*args, **kw)
            fake.calls.clear()
            fake.arrays.clear()

    cov = Dry()
    for seed in SEEDS:
        s = sequence_part(seed, cov, check=False, script=fake.script)
        assert s["n_bad"] == 0, s["first_bad"]                          # roster.table() is the State's after every step
        assert_the_counts(s["counts"], device=False)
    assert_the_coverage(cov.as_json())


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def sequence_run(built):
    res = child_run.run_child("device_sequence_child.py", "DEVICE_SEQUENCE", 300)
    print("\n[sequence]", json.dumps(res)[:6000])
    return res


@pytest.mark.gpu
def test_a_seeded_interleaving_matches_the_models_at_every_step(sequence_run):
    assert sequence_run["seeds"] == list(SEEDS) and len(sequence_run["sequence"]) == 2
    for s in sequence_run["sequence"]:
        caps = [r["capacity"] for r in s["rosters"]]
        assert sorted(caps) == sorted(CAPACITIES + (REPLACEMENT_CAPACITY,)) and {r["clones"] for r in s["rosters"]} == {1, 65}
        assert all(r["steps"] >= STEPS_PER_ROSTER for r in s["rosters"]), s["rosters"]
        # two rosters live at once, their steps alternating; one closed mid-run, its handle taken by a roster of another size
        assert s["handle_reused"] is True and s["alternated"] >= 2 * STEPS_PER_ROSTER
        c = s["counts"]
        assert c["recorded"] > 50 and c["told"] > 10 and c["relays"] > 50 and c["clone_senders"] > 10 and c["lines_compared"] > 100
        assert c["empty_texts"] > 0 and c["longest_text"] >= 999
        assert_the_counts(c, device=True)
        assert s["n_bad"] == 0, s["first_bad"]


@pytest.mark.gpu
def test_every_kind_ran_after_every_update_that_matters_to_it(sequence_run):
    assert_the_coverage(sequence_run["coverage"])


@pytest.mark.gpu
def test_go_many_passed_every_subset_of_its_kept_tables(sequence_run):
    """What the roster's flags said before each go_many call, for the calls the model agreed with: all 16 subsets of the
    speaker state, the clone records, the room table and the go table, {clones}, {speech} and {go} without rooms among them."""
    seen = sequence_run["coverage"]["go_subsets"]
    assert sorted(seen) == sorted(GO_SUBSETS) and all(n > 0 for n in seen.values()), seen


@pytest.mark.gpu
@pytest.mark.parametrize("kind", EVENT_KINDS)
def test_the_three_event_kinds_passed_every_subset_of_their_kept_tables(sequence_run, kind):
    """As go_many's sixteen, for the four kinds (the name is from when they were three): access_many, clone_many and act_many
    over the speaker state, the clone records, the room table and the go table -- act_many's speaker state on
    ``_private_dirty`` alone among them --; set_many over the speaker state, the AFK messages, the descriptions and the go table, each with the room table
    clean, dirty and passed by a call that holds a ``.topic``, and dirty and kept back by one that holds none."""
    seen = sequence_run["coverage"][f"{kind[:-5]}_subsets"]
    want = SET_SUBSETS if kind == "set_many" else GO_SUBSETS
    assert len(want) == (48 if kind == "set_many" else 16)
    assert sorted(seen) == sorted(want) and all(n > 0 for n in seen.values()), seen
    assert all(s["counts"]["act_private_alone"] > 0 for s in sequence_run["sequence"])


@pytest.mark.gpu
def test_a_regrown_allocation_gets_the_table_again_for_every_ordered_pair(sequence_run):
    """The first B after the small A finds the allocation freed and made anew, and uploads the table from the pinned mirror
    though the roster passed none: the table's two 256-byte aligned slices more than its repeat, and nothing else, for all
    182 ordered pairs of the fourteen table-reading kinds.  (On the MI355X every pair differs by exactly 768 bytes: layout_act
    brought no new finding, as layout_access, layout_clone, layout_set, layout_who, layout_rooms and layout_go had brought
    none.  The fresh roster has made a call of ten kinds: as B, plan_many, speak_many, input_many, tell_many, relay_many and
    clone_many need K = 16, act_many 32 behind every kind, access_many 32, or 64 behind plan_many, who_many and set_many
    64, go_many 64, or 32 behind rooms_many and clone_many, broadcast_many 128, look_many 16 to 64 by the A before it, and
    rooms_many, which grows by four bytes a looker, 39,232 to 43,264 lookers, the K its arithmetic starts from.  Before
    upload() of fanout.hip, 30 of
    the first 42 pairs copied the room behind the table as well: 2,048 bytes with speak_many or input_many as B, 6,400 with
    tell_many, 9,728 with look_many, 2,304 with relay_many, where 768 were due.)"""
    g = sequence_run["regrowth"]
    pairs = {f"{a}>{b}" for a in TABLE_KINDS for b in TABLE_KINDS if a != b}
    assert len(pairs) == 182 and set(g["pairs"]) == pairs and g["with_update"] == 182
    for pair, p in sorted(g["pairs"].items()):
        print(pair, p)
    assert g["table_slices"] == slice_of(4 * 65) + slice_of(65) == 768
    for pair, p in g["pairs"].items():
        assert p["first"] > p["repeat"] and p["first"] - p["repeat"] == g["table_slices"], (pair, p)
    assert g["n_bad"] == 0, g["first_bad"]
