"""The twelve device calls of ``device.Roster`` interleaved: the host mirrors and their dirty flags, the pending ring
clears, and the device allocation that is freed and made anew when a call needs more.

Host tier (unmarked): ``device._load`` is replaced by a library that computes nothing and records what it is passed.  A
seeded stream of updates, ``set_rooms``, ``set_clones``, clears and calls runs over one roster with every feature on, and
an independent model says which fields are stale on the device: an update makes its fields stale, passing a mirror to the
library cleans every field that lives in it.  After every call no field that call kind reads (``READS`` of
tests/device_sequence_child.py, from the kernels) may be stale, and a pending clear goes down with the first call that
touches its rings and with no later one.  ``go_many`` changes the mirrors itself: the fake library answers ``nd_roster_go``
from the model's ``go_call``, so the binding's apply step really runs, and the model makes stale what the model's call says
changed -- the table after a move, ``invite_room`` after a dropped invite, ``rooms.access`` and a pending review clear after
a room returned to public -- never what the roster says.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_sequence_child.py, under ``timeout``), and the tests assert on its JSON.
"""
from __future__ import annotations

import json
import random

import numpy as np
import pytest

import child_run
from device_sequence_child import (CAPACITIES, CLONE_FIELDS, FIELDS, GO_TABLES, KINDS, LOOK_ROOMS, MIRROR_OF, MIRRORS, READS,
                                   RECORDING_KINDS, RELAY_NAMES, REPLACEMENT_CAPACITY, REVIEW_ROOMS, ROOM_FIELDS, SEEDS,
                                   STEPS_PER_ROSTER, TABLE_FIELDS, TABLE_KINDS, UNREAD, USER_FIELDS, Coverage, Runner, State,
                                   clear_blocks, new_roster, op_for, random_op, sequence_part, slice_of)
from nuts333_amd import device

HOST_STEPS = 3000
#: the least a seed's device run counts, from the model's calls: see assert_the_counts
#: (the dry run counts 121 and 133 moves, 25 and 26 rooms returned, 295 and 384 deferred events, 6,810 and 7,138 who lines, 634
#: and 467 listings)
MOVES, RETURNED, DEFERRED, WHO_LINES, ROOMS_LISTINGS = 100, 20, 200, 5000, 400
#: where each entry point takes its pending clears, and the argument that says whether it records (None: it always
#: touches the rings); nd_roster_plan and nd_roster_relay take no clears and touch no ring, and neither do nd_roster_who,
#: nd_roster_rooms and nd_roster_go, whose argument lists hold the kept tables and the results alone: the clear a go_many
#: leaves behind goes down with a later call
CLEAR_AT = {"nd_roster_plan_record": (-1, None, False), "nd_roster_relay_record": (-1, None, False),
            "nd_roster_review": (3, None, False), "nd_roster_revtell": (3, None, True), "nd_roster_speak": (13, 10, False),
            "nd_roster_input": (11, 8, False), "nd_roster_tell": (13, 9, True)}
ENTRY_POINTS = {"broadcast_many": ("nd_roster_fanout",), "plan_many": ("nd_roster_plan", "nd_roster_plan_record"),
                "speak_many": ("nd_roster_speak",), "input_many": ("nd_roster_input",), "tell_many": ("nd_roster_tell",),
                "look_many": ("nd_roster_look",), "relay_many": ("nd_roster_relay", "nd_roster_relay_record"),
                "who_many": ("nd_roster_who",), "rooms_many": ("nd_roster_rooms",), "go_many": ("nd_roster_go",),
                "review_many": ("nd_roster_review",), "revtell_many": ("nd_roster_revtell",)}


# ------------------------------------------------------------------ a library that computes nothing
class FakeLibrary:
    """Every ``nd_roster_*`` call returns 0 and is kept in ``calls`` as ``(name, args)``.  ``arrays`` maps an address
    ``device._ptr`` handed out to its array, so that what an argument points at can be looked at.  ``nd_roster_go`` answers
    with the next entry of ``script``, per event ``(outcome, target, old_room, returned)``, as the fake library of
    tests/test_device_go.py does: the Runner puts the model's there."""

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
            if name == "nd_roster_go":                                  # outcome, target, old_room, returned; no text at all
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


# ------------------------------------------------------------------ which fields are stale on the device
class Host(Coverage):
    """The staleness model, fed by the Runner's steps and by what the fake library was passed."""

    def __init__(self, lib: FakeLibrary, roster: device.Roster, state: State):
        super().__init__()
        self.lib, self.roster, self.state = lib, roster, state
        self.stale = set(FIELDS)                                        # nothing is on the device yet
        self.stale_at_call = set()                                      # (kind, field) with the field stale when kind was called
        self.awaiting, self.read_clean_later = set(), set()             # (kind, unread stale field) pairs, and those confirmed
        self.masks = [np.zeros(REVIEW_ROOMS, dtype=np.uint8), np.zeros(state.cap, dtype=np.uint8)]
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

    def called(self, label, kind, review_rings, revtell_rings, go=None) -> None:
        super().called(label, kind, review_rings, revtell_rings, go)
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
                rings = [rm for rm in go["returned"] if rm < REVIEW_ROOMS]
                if rings:
                    self.masks[0][rings] = 1
                    self.clear_pending[0] = True
            touches = [False, False]
        else:
            assert len(calls) == 1, f"{self.step}: {kind} made {len(calls)} library calls"
            assert names[0] in ENTRY_POINTS[kind], f"{self.step}: {kind} went through {names[0]}"
            self.library_call(kind, *calls[0])
            touches = self.clears(*calls[0])
        assert touches == [bool(review_rings), bool(revtell_rings)], f"{self.step}: {names[0]} and the test disagree on the rings"
        self.lib.arrays.clear()

    def library_call(self, kind, name, args) -> None:
        """One library call of ``kind``: the mirrors it was passed are clean, and nothing it reads may be stale."""
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
        read_stale = sorted(READS[kind] & self.stale)
        assert not read_stale, (f"{self.step}: {kind} ({name}) read {read_stale} stale: it was passed {sorted(passed)}, dirty flags "
                                f"{ {f: getattr(self.roster, f) for f in ('_dirty', '_speech_dirty', '_private_dirty', '_afk_dirty', '_rooms_dirty', '_udesc_dirty', '_clones_dirty', '_who_dirty', '_go_dirty')} }")
        self.read_clean_later |= {(k, f) for k, f in self.awaiting if f in READS[kind]}
        self.awaiting |= {(kind, f) for f in before - READS[kind]}

    def clears(self, name, args) -> list:
        """The pending clears: down with the first call that records into, or reads, their rings, and with no later one.
        Returns which rings the call touches."""
        at = CLEAR_AT.get(name)
        touches = [False, False]
        if at is not None:
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
        rooms = [self.rng.randrange(REVIEW_ROOMS) for _ in range(self.rng.randint(1, 2))]
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
    for pair in (("vis", "afk"), ("name", "igntell"), ("level", "afk"), ("muzzled", "igntell")):
        blocks += [[("update", pair), (kind, {})] for kind in KINDS]
    blocks += [[("update", tuple(rng.sample(USER_FIELDS, n))), (kind, {})] for kind in KINDS for n in (2, 3, 6)]
    # afk and igntell alone, then a kind that reads the speaker mirror without them, then one that reads them: the mirror
    # is clean when the update comes, so only the flag of their own can bring it up
    blocks += [[("speak_many", {}), ("update", (f,)), (between, {}), (reader, {})] for f, readers in
               (("afk", ("tell_many", "look_many")), ("igntell", ("tell_many",))) for between in ("speak_many", "input_many")
               for reader in readers]
    # go_many's aftermath met first by every kind: a move with a dropped invite and a room returned to public
    blocks += [[("go_many", {"returns": True}), (kind, {})] for kind in KINDS]
    blocks += clear_blocks() * 3
    while sum(map(len, blocks)) < HOST_STEPS:
        blocks.append([random_op(rng)])
    rng.shuffle(blocks)
    return blocks


def host_run(lib, seed: int, ops=None, cap: int = 9, nclones: int = 4):
    rng = random.Random(seed)
    state = State(rng, cap, nclones)
    roster = new_roster(cap, nclones)
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
    assert set(MIRROR_OF.values()) == set(MIRRORS) | {"names"} and len(KINDS) == 12 and set(READS) == set(KINDS)
    assert KINDS[7:10] == ("who_many", "rooms_many", "go_many") and len(TABLE_KINDS) == 10
    assert set(TABLE_KINDS) == set(KINDS) - {"review_many", "revtell_many"}
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
    for f, kind in (("rooms.inlink", "rooms_many"), ("last_login", "who_many"), ("away", "who_many"), ("in_phrase", "go_many"),
                    ("out_phrase", "go_many"), ("invite_room", "go_many")):
        assert [k for k in KINDS if f in READS[k]] == [kind], f


def test_no_call_kind_ever_reads_a_stale_field(fake):
    host, runner, ops = host_run(fake, 20264)
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
    assert set(host.first_after_clear_review) == set(RECORDING_KINDS) | {"review_many"}
    assert set(host.first_after_clear_revtell) == {"tell_many", "revtell_many"}
    # ... a clear that a go_many left behind included
    assert set(host.first_after_go_clear) == set(RECORDING_KINDS) | {"review_many"}
    c = runner.counts
    # the blocks alone hold 27 go_many calls that move, drop an invite and return a room: one per kind, five clear blocks thrice
    assert c["moves"] >= 27 and c["returned_public"] >= 27 and c["invites_dropped"] >= 27 and c["deferred"] > 0, c
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
], ids=["afk-speak-look", "igntell-input-tell", "vis+afk", "name+igntell", "names-between-relays", "review-clear-waits",
        "revtell-clear-waits", "afk-rooms-go", "vis+afk-go-rooms", "go-moves-then-each", "go-returns-rooms-table", "who-table",
        "go-clear-waits"])
def test_the_rules_that_are_not_uniform_one_by_one(fake, ops):
    host, runner, _ = host_run(fake, 5, ops=ops)
    assert runner.steps == len(ops)


QUIET, RETURNS = ("go_many", {"quiet": True}), ("go_many", {"returns": True})


def was_passed(host, ops) -> list:
    """Per op that is a call, the mirrors its library call was passed; the look inside a go_many that moved is left out."""
    log, out = list(host.log), []
    for op in ops:
        if op[0] in KINDS:
            kind, passed = log.pop(0)
            assert kind == op[0]
            out.append(passed)
            if op == RETURNS:
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
    returned a room to public: the next go_many is passed the go table, and the room table unless a kind in between took it."""
    ops = [(k, {}) for k in TABLE_KINDS if k != "go_many"] + [QUIET, RETURNS, (kind, {}), QUIET, QUIET]
    host, runner, _ = host_run(fake, 5, ops=ops)
    passed = was_passed(host, ops)
    moved, nxt, later, last = passed[-4:]
    assert runner.counts["moves"] == 1 and runner.counts["invites_dropped"] >= 1 and runner.counts["returned_public"] == 1
    assert "_table" not in nxt and "_table" not in later
    assert ("_rooms" in nxt) == (kind in ("look_many", "who_many", "rooms_many"))      # the room table has one flag
    assert "_go" in later and ("_rooms" in later) == ("_rooms" not in nxt)
    assert last == frozenset()


def test_only_who_many_cleans_the_who_table(fake):
    ops = [("who_many", {}), ("look_many", {}), ("update", ("last_login",)), ("look_many", {}), ("who_many", {}), ("who_many", {})]
    host, _, _ = host_run(fake, 5, ops=ops)
    passed = was_passed(host, ops)
    assert "_who" in passed[0] and "_who" not in passed[3] and host.roster._who_dirty is False
    assert "_who" in passed[4] and "_who" not in passed[5]


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


def assert_the_counts(c: dict, device: bool) -> None:
    """What a seed's run counts of the three new kinds, from the model's calls.  The floors are those of a run of the
    child's streams over the library that computes nothing (the dry run below asserts them too), rounded down."""
    print(c)
    assert c["moves"] >= MOVES and c["returned_public"] >= RETURNED and c["deferred"] >= DEFERRED, c
    assert c["invites_dropped"] >= RETURNED and c["who_lines"] >= WHO_LINES and c["rooms_listings"] >= ROOMS_LISTINGS, c


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
    for kind in RECORDING_KINDS + ("review_many",):                    # the clear that a go_many left behind
        assert cov["first_after_go_clear"].get(kind, 0) > 0, kind
    assert sorted(cov["go_subsets"]) == sorted(GO_SUBSETS), sorted(set(GO_SUBSETS) - set(cov["go_subsets"]))


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
def test_a_regrown_allocation_gets_the_table_again_for_every_ordered_pair(sequence_run):
    """The first B after the small A finds the allocation freed and made anew, and uploads the table from the pinned mirror
    though the roster passed none: the table's two 256-byte aligned slices more than its repeat, and nothing else, for all
    90 ordered pairs of the ten table-reading kinds.  (On the MI355X every pair differs by exactly 768 bytes: layout_who,
    layout_rooms and layout_go brought no new finding.  The fresh roster has made a who_many, so the allocation to outgrow
    is larger than it was with seven kinds: as B, speak_many, input_many, tell_many and relay_many need K = 16, plan_many 32,
    go_many and who_many 64, broadcast_many 128, look_many 256, or 512 behind speak_many, and rooms_many, which grows by
    four bytes a looker, 49,664 or 50,496 lookers, the K its arithmetic starts from.  Before upload() of fanout.hip, 30 of
    the first 42 pairs copied the room behind the table as well: 2,048 bytes with speak_many or input_many as B, 6,400 with
    tell_many, 9,728 with look_many, 2,304 with relay_many, where 768 were due.)"""
    g = sequence_run["regrowth"]
    pairs = {f"{a}>{b}" for a in TABLE_KINDS for b in TABLE_KINDS if a != b}
    assert len(pairs) == 90 and set(g["pairs"]) == pairs and g["with_update"] == 90
    for pair, p in sorted(g["pairs"].items()):
        print(pair, p)
    assert g["table_slices"] == slice_of(4 * 65) + slice_of(65) == 768
    for pair, p in g["pairs"].items():
        assert p["first"] > p["repeat"] and p["first"] - p["repeat"] == g["table_slices"], (pair, p)
    assert g["n_bad"] == 0, g["first_bad"]
