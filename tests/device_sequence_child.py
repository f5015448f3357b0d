"""The device work of tests/test_device_sequence.py, in a short-lived child process of its own, and what the host tier of
that module shares with it: the state a sequence test owns, the fields every call kind reads, and the seeded step stream.

As tests/device_relay_child.py: the test module starts this script once, under ``timeout``, and asserts on the one JSON
line it prints (``DEVICE_SEQUENCE {...}``).  Every other ``device_*_child.py`` fuzzes one call kind on a roster it has just
built.  This one interleaves the sixteen device calls of a ``device.Roster`` with ``update``, ``set_rooms``, ``set_clones``,
``clear_review`` and ``clear_revtell`` on rosters that live long, two of them at once, and compares every call in full
with the models of those children, computed from a ``State`` kept here in plain Python and never from the roster's mirrors.
Five calls change the roster themselves: ``go_many``, ``access_many``, ``clone_many``, ``set_many`` and ``act_many``.  The
model's ``go_call``, ``access_call``, ``clone_call``, ``set_call`` or ``act_call`` changes the State as the call's apply step
changes the roster's mirrors -- the users' rooms and invitations, the rooms' access and topics, the clone records and where
they lie, the flags and texts a user sets of itself, the muzzle one user sets on another -- and the next call of any kind
meets what it left.  No call of the four breaks what the State promises every kind: none moves slot 0 out of the ring
rooms, takes its name or sets its login flag, and where a ``.destroy`` takes the last record the Runner makes record 0 anew
with a ``set_clones`` of its own.  ``regrowth_part`` makes, for every ordered pair of the fourteen table-reading kinds, 182
of them, a small call of the one and then a large call of the other, so that the second finds a device allocation that
was freed and made anew.

    python tests/device_sequence_child.py [--seed S] [--seed2 T]
"""
from __future__ import annotations

import argparse
import json
import random
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from device_access_child import EFFECTIVE as ACCESS_EFFECTIVE  # noqa: E402
from device_access_child import access_call, access_differences, access_events  # noqa: E402
from device_access_child import settings as access_settings  # noqa: E402
from device_act_child import EFFECTIVE as ACT_EFFECTIVE  # noqa: E402
from device_act_child import MOVED as ACT_MOVED  # noqa: E402
from device_act_child import act, act_call, act_differences, act_events, muzzle_differences  # noqa: E402
from device_clone_child import EFFECTIVE as CLONE_EFFECTIVE  # noqa: E402
from device_clone_child import clone_call, clone_differences, clone_events, record_differences, trim  # noqa: E402
from device_clone_child import settings as clone_settings  # noqa: E402
from device_fanout_child import fuzz_items  # noqa: E402
from device_go_child import MOVED, WIZ, WORST_PHRASES, fuzz_events, go, go_call, go_differences, mirror_differences  # noqa: E402
from device_input_child import answer_of, fuzz_read, input_differences  # noqa: E402
from device_input_child import new_counts as input_counts  # noqa: E402
from device_look_child import WORST_DESCS, WORST_NAMES, fuzz_rooms, look_differences  # noqa: E402
from device_look_child import new_counts as look_counts  # noqa: E402
from device_many_child import COMS as BROADCAST_COMS  # noqa: E402
from device_many_child import Cpu, compare, expected, table  # noqa: E402
from device_plan_child import plan_differences  # noqa: E402
from device_relay_child import ALL, NOTHING, SWEARS, longest_text, relay_text, relays  # noqa: E402
from device_review_child import Rings, review_differences  # noqa: E402
from device_rooms_child import rooms_differences  # noqa: E402
from device_roster_child import Model  # noqa: E402
from device_set_child import EFFECTIVE as SET_EFFECTIVE  # noqa: E402
from device_set_child import fuzz_events as set_events  # noqa: E402
from device_set_child import mirror_differences as set_mirror_differences  # noqa: E402
from device_set_child import set_call, set_differences  # noqa: E402
from device_speak_child import COMS as SPEECH_COMS  # noqa: E402
from device_speak_child import EMOTE, SAY, fuzz_inpstr, model, speech_differences  # noqa: E402
from device_tell_child import COMS as TELL_COMS  # noqa: E402
from device_tell_child import TOLD, TellRings, fuzz_event, new_user, private, private_differences  # noqa: E402
from device_tell_child import new_counts as tell_counts  # noqa: E402
from device_who_child import QUIRK_DESCS, QUIRK_NAMES, bits_of, listed, who_differences  # noqa: E402
from device_who_child import new_counts as who_counts  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402

KINDS = ("broadcast_many", "plan_many", "speak_many", "input_many", "tell_many", "look_many", "relay_many", "who_many",
         "rooms_many", "go_many", "access_many", "clone_many", "set_many", "act_many", "review_many", "revtell_many")
#: the kinds whose kernels read the table (nd_roster_review and nd_roster_revtell neither read nor upload it)
TABLE_KINDS = KINDS[:14]
#: the four whose apply step changes the mirrors as go_many's does, compared and counted alike
EVENT_KINDS = ("access_many", "clone_many", "set_many", "act_many")
#: the kinds that can record into the rooms' review rings, and the two that touch the slots' revtell rings; clone_many
#: records only on a roster whose every look room has a ring (State.records_clones)
RECORDING_KINDS = ("plan_many", "speak_many", "input_many", "relay_many")
#: the ring rooms of a State and its roster unless it is made with another number; LOOK_ROOMS of them let clone_many record
REVIEW_ROOMS, LOOK_ROOMS = 3, 5
CAPACITIES = (1, 64, 65, 257)
#: the roster made in the closed one's place
REPLACEMENT_CAPACITY = 130
STEPS_PER_ROSTER = 400
#: the seeds of the device run, and of the host tier's dry run of the same streams
SEEDS = (20262, 20263)
#: the rooms a roomless user may be away over: State keeps a netlink that is UP on both, whatever set_rooms draws
AWAY_ROOMS = (0, 3)
#: no last_login is later, and every who_many is asked at or after it
NOW = 1_000_000
DATE = b"on Monday 19 October 2026 at 00:07"
#: the lookers of a who_many or rooms_many past this many repeat the first ones
PERIOD = 16
#: a word that begins no room's name and no netlink's service: a go_many of such events moves nobody
NOWHERE = b"zzq"

# ------------------------------------------------------------------ the fields, and where each lives
TABLE_FIELDS = ("room", "login", "ignall", "ignshout", "colour")
SPEECH_FIELDS = ("name", "vis", "muzzled", "muzzle_level", "command_mode", "level", "afk", "igntell", "prompt", "charmode_echo")
WHO_FIELDS = ("last_login", "away")
GO_FIELDS = ("in_phrase", "out_phrase", "invite_room")
USER_FIELDS = TABLE_FIELDS + SPEECH_FIELDS + ("afk_mesg", "desc") + WHO_FIELDS + GO_FIELDS
ROOM_FIELDS = ("name", "access", "desc", "links", "topic", "mesg_cnt", "netlink", "inlink")
#: the key of a user's dict where it is not the field's name: go_user's, and act_user's
KEY = {"invite_room": "invite", "muzzle_level": "muzzle"}
#: Roster.update refuses the two in one call: muzzle_level writes the muzzled bit too
MUZZLE_FIELDS = ("muzzled", "muzzle_level")
CLONE_FIELDS = ("owner", "room", "hear")
#: the rooms' names as relay_many keeps them: no host mirror of the roster, an array it builds per call and compares
RELAY_NAMES = "relay.names"
#: field -> the mirror it lives in (an attribute of device.Roster, or "names" for the array of relay_many)
MIRROR_OF = {**{f: "_table" for f in TABLE_FIELDS}, **{f: "_speech" for f in SPEECH_FIELDS}, "afk_mesg": "_afk", "desc": "_udesc",
             **{f: "_who" for f in WHO_FIELDS}, **{f: "_go" for f in GO_FIELDS},
             **{f"rooms.{f}": "_rooms" for f in ROOM_FIELDS}, **{f"clones.{f}": "_clones" for f in CLONE_FIELDS},
             RELAY_NAMES: "names"}
FIELDS = tuple(MIRROR_OF)
MIRRORS = ("_table", "_speech", "_afk", "_rooms", "_udesc", "_clones", "_who", "_go")

_TABLE = frozenset(TABLE_FIELDS)
#: What each call kind reads, from the kernels of nuts333_amd/device/fanout.hip and their nd_roster_* entry points (the
#: functions named are those kernels' bodies; an entry point hands a kernel the uploaded table or the kept one, never both).
#: The table is one mirror with one flag, so a kind that reads one of its fields is listed with all five: colour is read
#: on the host as well, by every kind that returns a Plan's colour_bits or a Look's colour.
READS = {
    # nd_roster_fanout -> roster_measure / roster_emit: listener_record(a.room[j], a.slot[j], ...) in roster_measure, the
    # colour bit of a.slot[j] picks the variant in roster_emit
    "broadcast_many": _TABLE,
    # plan_call -> roster_plan: listener_record(a.room[j], a.slot[j], ...)
    "plan_many": _TABLE,
    # speech_call -> roster_speak: a.room[slot]; of the speaker's 16 bytes the name and its length, muzzled, command_mode
    # and vis; roster_speak_plan: listener_record.  Neither reads the level byte nor the afk and igntell bits
    "speak_many": _TABLE | {"name", "vis", "muzzled", "command_mode"},
    # ... and roster_parse in front of them: command_mode and the level byte
    "input_many": _TABLE | {"name", "vis", "muzzled", "command_mode", "level"},
    # nd_roster_tell -> roster_tell: the speaker's name, muzzled and vis; get_user over every slot's login flag and name
    # (name_match); both levels; the target's afk, ignall, igntell, room and name; its AFK message.  It reads the level,
    # which the issue's table of this test did not expect and update()'s docstring does not say; it does not read
    # command_mode
    "tell_many": _TABLE | {"name", "vis", "muzzled", "level", "afk", "igntell", "afk_mesg"},
    # nd_roster_look -> roster_look: a.room[j], the looker's level, every slot's name, vis and level; look_line: vis, the
    # description, afk; look_room: the whole room record but its inlink bit, which only roster_rooms_lines tests
    "look_many": _TABLE | {"name", "vis", "level", "afk", "desc"} | {f"rooms.{f}" for f in ROOM_FIELDS if f != "inlink"},
    # relay_call -> roster_plan, roster_relay: the records' owner, room and hear, the owner's ignall, the room's name from
    # the 24-byte rows and nothing else of the room table
    "relay_many": _TABLE | {f"clones.{f}" for f in CLONE_FIELDS} | {RELAY_NAMES},
    # nd_roster_who -> roster_who: a.room[j] and the login flag of every slot; of the speaker's 16 bytes the name and its
    # length, vis and the level (roster_who_shown: the looker's level too); who_line: the description, afk; the who row's
    # last_login, and its away where the slot has no room.  Of the room record it prints the name, or the netlink's
    # service behind the '@', and nothing else: not the access, the topic or the links
    "who_many": _TABLE | {"name", "vis", "level", "afk", "desc", "last_login", "away", "rooms.name", "rooms.netlink"},
    # nd_roster_rooms -> roster_rooms_count: a.room[j], the login flag, and of the speaker's 16 bytes the name's length
    # alone; roster_rooms_lines: the record's name, access, mesg_cnt, topic, and the net byte (netlink and inlink) with
    # the service
    "rooms_many": _TABLE | {"name"} | {f"rooms.{f}" for f in ("name", "access", "topic", "mesg_cnt", "netlink", "inlink")},
    # nd_roster_go -> roster_go: a.room[slot], and for who stays behind every slot's room, login flag and name length;
    # the mover's name, vis and level; the go row's two phrases and invite_room; the mover's room record's netlink, links
    # and access, every record's name, the target's access.  Of a clone record it reads the owner and the room: who hears
    # what plays no part in reset_access, so hear is not read, though the issue's table expected the whole record.
    # roster_speak_plan: listener_record
    "go_many": _TABLE | {"name", "vis", "level", "clones.owner", "clones.room", "in_phrase", "out_phrase", "invite_room"}
               | {f"rooms.{f}" for f in ("name", "access", "links", "netlink")},
    # nd_roster_access -> roster_access: a.room[slot], and for the head-count of a .private every slot's room, login flag
    # and name length; the actor's name, vis and level; wave_get_user over every slot's login flag and name, the found
    # slot's room and its invite_room; wave_get_room over every record's name (its name length and bytes, nothing of the
    # netlink, which the issue's table of this test left open); the actor's room's access and links, the target's access
    # and name.  Of a clone record the owner and the room.  order_events<AccessOrderArgs>: a.room again.
    # roster_speak_plan: listener_record
    "access_many": _TABLE | {"name", "vis", "level", "clones.owner", "clones.room", "invite_room"}
                   | {f"rooms.{f}" for f in ("name", "access", "links")},
    # nd_roster_clone -> roster_clone: c.room[slot]; the actor's name, vis, level and muzzled; wave_get_user (.destroy
    # <room> <name>) and the found owner's level and name; wave_get_room; the target's access and name; the actor's
    # invite_room (has_room_access); the records' owner and room (the walk, create_clone's two counts, wave_head_count with
    # every slot's room, login flag and name length).  No kernel reads hear: a .chear's value is set on the host, so "all
    # three fields", as the issue's table expected, is one too many.  roster_speak_plan: listener_record
    "clone_many": _TABLE | {"name", "vis", "level", "muzzled", "clones.owner", "clones.room", "invite_room", "rooms.name",
                            "rooms.access"},
    # nd_roster_set -> roster_set: a.room[slot] and the actor's flag byte of the table (ignall, ignshout, colour); of its 16
    # speaker bytes the name, vis, command_mode, igntell, prompt and charmode_echo -- not the afk bit, though SetArgs'
    # comment lists it, and neither muzzled nor the level; its description (.desc), AFK message (.afk without one) and two
    # phrases; a.rooms only under com == kComTopic, and nd_roster_set hands it the room table only when the call holds a
    # .topic: rooms.topic is read by such a call alone (reads_of).  roster_speak_plan: listener_record
    "set_many": _TABLE | {"name", "vis", "command_mode", "igntell", "prompt", "charmode_echo", "afk_mesg", "desc", "in_phrase",
                          "out_phrase", "rooms.topic"},
    # nd_roster_act -> roster_act: a.room[slot] and a.room[target]; wave_get_user over every slot's login flag and name;
    # wave_get_room over every record's name; of the actor's 16 speaker bytes the name, vis, the level and muzzled (a muzzled
    # waker); of the target's the name, vis, the level, afk (.wake), muzzled and byte 15, the muzzle's level; the actor's
    # invite_room (has_room_access); the resolved room's access and name and the access of the room left; the head count of
    # the room left over every slot's room, login flag and name length and the records' owner and room.
    # order_events<ActOrderArgs>: a.room again.  roster_speak_plan: listener_record.  As the issue's table of this test
    # expected, and of what it left open neither: the kernel reads no links -- the deferral over them is the binding's, from
    # the host mirror -- and nothing of a netlink: ACT_MOVE_AWAY is decided by the target's room index
    "act_many": _TABLE | {"name", "vis", "level", "muzzled", "muzzle_level", "afk", "invite_room", "clones.owner", "clones.room",
                          "rooms.name", "rooms.access"},
    # review_call: its layout steps over the table (layout_review), the kernel reads the rings alone
    "review_many": frozenset(),
    "revtell_many": frozenset(),
}
#: what of READS a call reads only when it holds a .topic
TOPIC_READS = frozenset({"rooms.topic"})


def reads_of(kind: str, topic: bool = False) -> frozenset:
    """What one call reads: READS of its kind, and for a set_many the room's topic only when the call holds a ``.topic``."""
    return READS[kind] if kind != "set_many" or topic else READS[kind] - TOPIC_READS


#: a field each kind does not read, for the step "an update of only fields it does not read"
UNREAD = {"broadcast_many": "desc", "plan_many": "name", "speak_many": "afk", "input_many": "igntell", "tell_many": "desc",
          "look_many": "muzzled", "relay_many": "level", "who_many": "rooms.access", "rooms_many": "afk", "go_many": "clones.hear",
          "access_many": "rooms.netlink", "clone_many": "clones.hear", "set_many": "afk", "act_many": "desc", "review_many": "room",
          "revtell_many": "colour"}

ROOM_NAME_POOL = (b"d", b"N" * 20, b"hallway", b"~FRred/", b"wiz", b"R" * 20, b"alone", b"pair", b"e", b"/~", b"drive")
SYLLABLES = (b"al", b"ice", b"bob", b"by", b"car", b"ol", b"dave", b"x", b"Zed", b"9", b"\xe9", b"an", b"na")
AFK_MESGS = (b"", b"", b"back in five", b"m" * 60, b"~FRred~RS \xe9")


def slice_of(n: int) -> int:
    """An array's 256-byte aligned slice of an upload (Carver of fanout.hip)."""
    return -(-n // 256) * 256


def apart(fields) -> tuple:
    """``fields`` without the second of MUZZLE_FIELDS where it holds both."""
    both = [f for f in fields if f in MUZZLE_FIELDS]
    return tuple(f for f in fields if f not in both[1:])


def written(fields) -> list:
    """The fields an update of ``fields`` writes: a muzzle's level writes the muzzled bit as well."""
    return list(fields) + ["muzzled"] * ("muzzle_level" in fields and "muzzled" not in fields)


def op_for(field: str) -> tuple:
    """The step that updates ``field`` and nothing else that lives elsewhere."""
    if field == RELAY_NAMES:
        return ("set_rooms", ("name",))
    if field.startswith("rooms."):
        return ("set_rooms", (field[6:],))
    if field.startswith("clones."):
        return ("set_clones", (field[7:],))
    return ("update", (field,))


# ------------------------------------------------------------------ the state the test owns
class State:
    """The truth, in plain Python: a dict per slot, the room records, the clone records as ``[owner, room, hear]`` (owner
    None: an empty record) and both sets of rings.  Slot 0 is always a speaker in a ring room and record 0 always owned, so
    that every call kind has somebody to call it for.  ``review_rooms`` is how many of the LOOK_ROOMS have a review ring,
    here and in the roster made for it (new_roster): with all of them, clone_many may record."""

    def __init__(self, rng: random.Random, cap: int, nclones: int, review_rooms: int = REVIEW_ROOMS):
        self.cap, self.nclones, self.review_rooms = cap, nclones, review_rooms
        self.rooms = fuzz_rooms(rng)                                     # AWAY_ROOMS have a netlink that is UP in these
        for rm in self.rooms:
            rm["inlink"] = rng.random() < 0.5
        self.users = {j: new_user(j, ignshout=0, desc=b"", last_login=0, away=AWAY_ROOMS[0], in_phrase=b"enters", out_phrase=b"goes",
                                  invite=None) for j in range(cap)}
        for j, u in self.users.items():
            for f in USER_FIELDS:
                u[KEY.get(f, f)] = self.value(rng, f, j)
            if u["muzzle"]:
                u["muzzled"] = 1                                         # a muzzle of a level is a muzzle: seat() can make it
            if j and rng.random() < 0.1:
                u["name"] = None                                         # a slot that never got a name
        self.records = []
        for c in range(nclones):
            empty = c > 0 and rng.random() < 0.15
            self.records.append([None, None, NOTHING] if empty else
                                [rng.randrange(cap), rng.randrange(4), rng.choice((NOTHING, SWEARS, ALL, ALL))])
        self.rings, self.tell_rings = Rings(review_rooms), TellRings(cap)

    def value(self, rng: random.Random, f: str, slot: int):
        if f == "room":
            return rng.choice((0, 1, 2)) if slot == 0 else rng.choice((0, 0, 1, 2, 3, 4, None))
        if f == "login":
            return 0 if slot == 0 else int(rng.random() < 0.1)
        if f == "name":
            x = rng.random()
            if x < 0.5:
                name = b"".join(rng.choice(SYLLABLES) for _ in range(rng.randrange(1, 5)))[:rng.choice((12, 12, 5, 3))]
                return name[:1].upper() + name[1:] if rng.random() < 0.8 else name
            return rng.choice(WORST_NAMES + QUIRK_NAMES) if x < 0.65 else b"Q%d" % slot
        if f == "level":
            return rng.randrange(5)
        if f == "afk_mesg":
            return rng.choice(AFK_MESGS)
        if f == "desc":
            return rng.choice(WORST_DESCS + QUIRK_DESCS)
        if f == "last_login":                                           # who()'s mins: 0, the edges of a minute and an hour, years
            return rng.choice((0, NOW, NOW - 59, NOW - 61, NOW - 3599, rng.randrange(NOW + 1)))
        if f == "away":
            # who() prints it only for a user without a room, and refuses such a user without one; room and away are
            # updated apart here, so every slot keeps an away
            return rng.choice(AWAY_ROOMS)
        if f in ("in_phrase", "out_phrase"):
            return rng.choice(WORST_PHRASES + ((b"enters", b"strolls in") if f == "in_phrase" else (b"goes", b"wanders off")))
        if f == "invite_room":
            return rng.choice((None, None, 0, 1, 2, 3, 4))
        if f == "muzzle_level":                                         # none most often; a GOD's, which a WIZ cannot remove
            return rng.choice((0, 0, 0, 0, 0, 0, 1, 2, 3, device.MAX_LEVEL, device.MAX_LEVEL))
        chance = {"ignall": 0.2, "ignshout": 0.3, "colour": 0.5, "vis": 0.7, "muzzled": 0.1, "command_mode": 0.3, "afk": 0.15,
                  "igntell": 0.2, "prompt": 0.3, "charmode_echo": 0.3}[f]
        return int(rng.random() < chance)

    def room_value(self, rng: random.Random, f: str, rm: int):
        if f == "name":
            return rng.choice([n for n in ROOM_NAME_POOL if n != self.rooms[rm]["name"]])
        if f == "access":
            return rng.randrange(4)
        if f == "desc":
            return rng.choice((b"\n" * 810, b"~FR" * 270, b"/~" * 405, b"", b"A room.\nWith ~OLtwo~RS lines and a slash/\n"))
        if f == "links":
            return [rng.randrange(LOOK_ROOMS) for _ in range(rng.choice((0, 1, 3, 10)))]
        if f == "topic":
            return rng.choice((b"", b"t" * 60, b"~OLbold~RS /~FR \xe9", b"a topic"))
        if f == "mesg_cnt":
            return rng.choice((0, 7, 2**31 - 1, rng.randrange(1000)))
        if f == "inlink":
            return not self.rooms[rm]["inlink"]
        # (service, allow_in) is a link that is UP, as look()'s and who()'s models take it; with a state .rmsn tells the three
        # apart, go() knows the link whatever its state and look() only when it is UP (look_of).  An away room stays UP
        up = ((b"s" * 80, True), (b"peer2", False), (b"in", True), (b"faraway", False, device.LINK_UP))
        if rm in AWAY_ROOMS:
            return rng.choice(up)
        return rng.choice((None, (b"far", True, device.LINK_DOWN), (b"s" * 80, False, device.LINK_VERIFYING)) + up)

    def seat(self, roster: device.Roster) -> None:
        """A roster that has just been made, in this state: the rooms first, update(away=) wants a room with a link.  The
        muzzles as seat_all of tests/device_act_child.py seats them: the level, which writes the bit too, then the bit alone
        where the level left another -- a muzzle without a level, or a level whose bit an update of ``muzzled`` took."""
        ids = list(range(LOOK_ROOMS))
        roster.set_rooms(ids, **{f: [self.rooms[i][f] for i in ids] for f in ROOM_FIELDS})
        slots = list(range(self.cap))
        roster.update(slots, **{f: [self.users[j][KEY.get(f, f)] for j in slots] for f in USER_FIELDS if f not in ("name", "muzzled")})
        bits = [j for j in slots if bool(self.users[j]["muzzled"]) != bool(self.users[j]["muzzle"])]
        if bits:
            roster.update(bits, muzzled=[self.users[j]["muzzled"] for j in bits])
        named = [j for j in slots if self.users[j]["name"]]
        roster.update(named, name=[self.users[j]["name"] for j in named])
        for c, (owner, room, hear) in enumerate(self.records):
            if owner is not None:
                roster.set_clones(c, owner=owner, room=room, hear=hear)

    def table_model(self) -> Model:
        m = Model(self.cap)
        for j, u in self.users.items():
            m.room[j] = -1 if u["room"] is None else u["room"]
            for f in m.flags:
                m.flags[f][j] = u[f]
        return m

    def speakers(self, ring: bool = False) -> list:
        """The slots that may speak: a room, no login flag, a name; ``ring``: and their room has a review ring."""
        return [j for j, u in self.users.items() if u["room"] is not None and not u["login"] and u["name"]
                and (not ring or u["room"] < self.review_rooms)]

    @property
    def records_clones(self) -> bool:
        """clone_many(record=True) wants a ring for every look room."""
        return self.review_rooms >= LOOK_ROOMS

    def take_clones(self, clones) -> None:
        """The records as clone_call left them (tuples, None for an empty one), back into the State's lists."""
        self.records = [[None, None, NOTHING] if c is None else list(c) for c in clones]

    def snapshot(self) -> dict:
        """Every field's values, to be compared after a model's call (changed_since)."""
        out = {f: [u[KEY.get(f, f)] for u in self.users.values()] for f in USER_FIELDS}
        out.update({f"rooms.{f}": [rm[f] if f != "links" else list(rm[f]) for rm in self.rooms] for f in ROOM_FIELDS})
        out.update({f"clones.{f}": [r[i] for r in self.records] for i, f in enumerate(CLONE_FIELDS)})
        return out

    def changed_since(self, before: dict) -> set:
        """The fields a model's call changed: what is stale on the device after the roster's call, whatever the roster says."""
        now = self.snapshot()
        return {f for f in now if now[f] != before[f]}

    def relay_records(self) -> list:
        return [tuple(r) for r in self.records]

    def cloned_rooms(self) -> set:
        return {r[1] for r in self.records if r[0] is not None}

    def go_clones(self) -> list:
        """The records as go_call's population() counts them: None for an empty one."""
        return [None if r[0] is None else tuple(r) for r in self.records]

    def seen_rooms(self) -> list:
        """The rooms as look() sees them: a netlink only when it is UP."""
        return [rm if rm["netlink"] is None or len(rm["netlink"]) < 3 or rm["netlink"][2] == device.LINK_UP else {**rm, "netlink": None}
                for rm in self.rooms]


# ------------------------------------------------------------------ what a run counts
class Coverage:
    """Which call kind ran directly after which update, and which was the first to touch the rings after a clear."""

    #: the calls whose apply step can return a ring room to public, and so leave a review clear pending
    CLEAR_SOURCES = {"go_many": "go", "access_many": "access", "clone_many": "clone", "act_many": "act"}

    def __init__(self):
        self.runs, self.after_read, self.after_unread = {}, {}, {}
        self.first_after_clear_review, self.first_after_clear_revtell = {}, {}
        #: ... after a clear that a go_many, an access_many, a clone_many or an act_many left; label -> the source of the
        #: pending one
        self.first_after = {source: {} for source in self.CLEAR_SOURCES.values()}
        self.clear_from = {}
        self.last = {}                                                   # roster label -> fields of the step just before
        self.pending = {}                                                # roster label -> [review clear, revtell clear]
        #: kind -> the kept tables a call of it passed -> calls the model agreed with
        self.subsets = {kind: {} for kind in ("go_many",) + EVENT_KINDS}

    def passed(self, kind: str, subset) -> None:
        key = "+".join(subset)
        self.subsets[kind][key] = self.subsets[kind].get(key, 0) + 1

    def updated(self, label: str, fields) -> None:
        self.last[label] = set(fields)

    def cleared(self, label: str, tell: bool) -> None:
        self.last.pop(label, None)
        self.pending.setdefault(label, [False, False])[int(tell)] = True

    def called(self, label: str, kind: str, review_rings: bool, revtell_rings: bool, go: dict | None = None,
               change: dict | None = None, reads=None) -> None:
        """``review_rings`` / ``revtell_rings``: the call records into, or reads, those rings.  ``go``: what the model says a
        go_many changed -- ``moved``, ``invites_dropped``, and ``rings``, the ring rooms that went back to public; one of
        those leaves a review clear pending, as clear_review does.  ``change``: the same of an access_many, a clone_many, a
        set_many or an act_many -- ``stale``, the fields the model's call changed, and ``rings``; of an act_many ``moved`` too.  ``reads``: what this call reads, where
        that is not READS of its kind (reads_of)."""
        reads = READS[kind] if reads is None else reads
        per = self.runs.setdefault(label, {k: 0 for k in KINDS})
        per[kind] += 1
        last = self.last.pop(label, None)
        if last:
            for f in last & reads:
                self.after_read[f"{kind}/{f}"] = self.after_read.get(f"{kind}/{f}", 0) + 1
            if not last & reads:
                self.after_unread[kind] = self.after_unread.get(kind, 0) + 1
        pending = self.pending.setdefault(label, [False, False])
        for i, (touches, first) in enumerate(((review_rings, self.first_after_clear_review),
                                              (revtell_rings, self.first_after_clear_revtell))):
            if touches and pending[i]:
                first[kind] = first.get(kind, 0) + 1
                source = self.clear_from.get(label)
                if i == 0 and source:
                    self.first_after[source][kind] = self.first_after[source].get(kind, 0) + 1
                pending[i] = False
                if i == 0:
                    self.clear_from[label] = None
        if (go or change or {}).get("rings"):
            pending[0], self.clear_from[label] = True, self.CLEAR_SOURCES[kind]

    def as_json(self) -> dict:
        return {"runs": self.runs, "after_read": self.after_read, "after_unread": self.after_unread,
                "first_after_clear_review": self.first_after_clear_review,
                "first_after_clear_revtell": self.first_after_clear_revtell,
                **{f"first_after_{source}_clear": first for source, first in self.first_after.items()},
                "go_subsets": self.subsets["go_many"], **{f"{kind[:-5]}_subsets": self.subsets[kind] for kind in EVENT_KINDS}}


#: what a run counts of access_many, clone_many, set_many and act_many, from the model's calls alone: per kind the effective
#: and the deferred events; the rooms an access call set private or returned to public, and those a destroy returned; the
#: records created and destroyed, the calls after which records moved down, the said lines a recording call stored; the set
#: calls that held a .topic, and those that held none while the roster's room table was dirty; the targets an act call
#: moved, the rooms it returned to public, the invitations its moves and returns cleared, the muzzles set and removed, the
#: wake-up calls sent and those refused for an AFK target, the muzzles that were above their remover -- and, from the
#: roster's flags before the call, the act calls that passed the speaker state on _private_dirty alone
EVENT_COUNTS = tuple(f"{kind[:-5]}_{what}" for what in ("effective", "deferred") for kind in EVENT_KINDS) + (
    "set_private", "access_returned", "destroy_returned", "created", "destroyed", "compacted", "said_recorded", "topic_calls",
    "topicless_dirty", "act_moved", "act_returned", "act_invites_cleared", "act_muzzled", "act_unmuzzled", "act_woken",
    "act_wake_afk", "act_unmuzzle_above", "act_private_alone")
#: set_many's kept tables in layout order; the room table is passed only by a call that holds a .topic, else kept back
SET_TABLES = ("speech", "afk", "udesc", "go", "rooms")
KEPT_BACK = "rooms-kept-back"


def text_of(rng: random.Random, lo: int, hi: int) -> bytes:
    """A text of lo .. hi bytes from fuzz_inpstr's kinds, without a NUL."""
    n, t = rng.randint(lo, hi), b""
    while len(t) < n:
        t += fuzz_inpstr(rng) + b" "
    return t[:n]


# ------------------------------------------------------------------ one roster, its state, and the steps
class Runner:
    """Makes steps on ``roster`` and on ``state`` alike.  With ``check`` every call's result is compared with the models
    (``bad`` collects what differs); without, only the calls are made, for a library that computes nothing -- and after an
    access_many, a clone_many, a set_many or an act_many, whose apply step is the binding's own, the roster's mirrors are still compared
    with the State.  ``seen`` is told of every step: ``updated(label, fields)``, ``cleared(label, tell)``, ``called(label,
    kind, review, revtell)`` with what the model says a call changed."""

    def __init__(self, rng: random.Random, roster: device.Roster, state: State, label: str, seen, check: bool = True,
                 cpu: Cpu | None = None, pool=None, script: list | None = None):
        self.rng, self.roster, self.state, self.label, self.seen, self.check = rng, roster, state, label, seen, check
        #: where a library that computes nothing finds what nd_roster_go answers: the model's, per event
        #: ``(outcome, target, old_room, returned)``
        self.script = script
        self.cpu = cpu or Cpu()
        self.pool = pool or [t for t, _ in fuzz_items(rng.randrange(1 << 30), 200)] + [b"", b"x" * 999, b"\n" * 999]
        self.bad, self.steps, self.cache, self.renamed = [], 0, {}, 0
        self.counts = {"input": input_counts(), "tell": tell_counts(), "look": look_counts(), "speech": {},
                       "review": {"rooms_reviewed": 0, "lines_compared": 0, "sequential_lines": 0, "wave_lines": 0},
                       "recorded": 0, "told": 0, "relays": 0, "clone_senders": 0, "longest_text": 0, "empty_texts": 0,
                       "who": who_counts(), "rooms": {"colours": set(), "empty": 0, "single": 0, "all": 0, "uncounted": 0,
                                                      "nameless_rooms": 0, "states": set(), "inlinks": set(), "fixed": 0},
                       # from the model alone, so that a run over a library that computes nothing counts the same
                       "moves": 0, "returned_public": 0, "deferred": 0, "invites_dropped": 0, "who_lines": 0, "rooms_listings": 0,
                       **{name: 0 for name in EVENT_COUNTS}}
        self.last_timing = {}
        #: the most bytes a call of this roster copied both ways: about what its allocation holds beside the tables
        self.largest = 0

    # -------------------------------------------------------------- updates
    def step(self, op: tuple) -> None:
        what, arg = op[0], op[1] if len(op) > 1 else None
        getattr(self, "_" + what)(arg if arg is not None else ({} if what in KINDS else ()))
        self.steps += 1
        self.table_is_the_states()

    def table_is_the_states(self) -> None:
        """roster.table() reads the roster's own mirror: speech_differences and input_differences admit through it, so it
        has to be the table the state gives."""
        want = table(self.state.table_model().records(None, None))
        if not np.array_equal(self.roster.table(None, None), want):
            self.bad.append({"step": self.steps, "what": "roster.table() is not the state's table"})

    def _update(self, fields) -> None:
        """``muzzled`` and ``muzzle_level`` never in one update, which the roster refuses: the second of them is dropped."""
        rng, st = self.rng, self.state
        fields = apart(fields)
        slots = [rng.randrange(st.cap) for _ in range(rng.randint(1, 4))]
        values = {f: [st.value(rng, f, j) for j in slots] for f in fields}
        self.roster.update(slots, **values)
        for i, j in enumerate(slots):                                   # in order: the last value wins
            for f in fields:
                self._took(j, f, values[f][i])
        self.seen.updated(self.label, written(fields))

    def _took(self, slot: int, f: str, value) -> None:
        """The State after an update of one field of one slot: a muzzle's level writes the muzzled bit too, the bit alone
        leaves the level as it was."""
        u = self.state.users[slot]
        u[KEY.get(f, f)] = value
        if f == "muzzle_level":
            u["muzzled"] = int(value != 0)

    def _set_rooms(self, fields) -> None:
        rng, st = self.rng, self.state
        rooms = rng.sample(range(LOOK_ROOMS), rng.randint(1, 2))
        values = {f: [st.room_value(rng, f, rm) for rm in rooms] for f in fields}
        self.roster.set_rooms(rooms, **values)
        for i, rm in enumerate(rooms):
            for f in fields:
                st.rooms[rm][f] = values[f][i]
        self.seen.updated(self.label, [f"rooms.{f}" for f in fields] + ([RELAY_NAMES] if "name" in fields else []))

    def _set_clones(self, fields, at: int | None = None) -> None:
        """``owner`` alone gives an owned record another owner, and CLONE_HEAR_ALL with it; ``room`` or ``hear`` alone change
        an owned record; all three make a record anew, or (owner None) empty it."""
        rng, st = self.rng, self.state
        owned = [c for c, r in enumerate(st.records) if r[0] is not None]
        if set(fields) == set(CLONE_FIELDS):
            c = rng.randrange(st.nclones) if at is None else at
            if c and rng.random() < 0.25:
                self.roster.set_clones(c, owner=None)
                st.records[c] = [None, None, NOTHING]
            else:
                st.records[c] = [rng.randrange(st.cap), rng.randrange(4), rng.choice((NOTHING, SWEARS, ALL))]
                self.roster.set_clones(c, owner=st.records[c][0], room=st.records[c][1], hear=st.records[c][2])
        else:
            c = rng.choice(owned)
            new = {"owner": rng.randrange(st.cap), "room": rng.randrange(4), "hear": rng.choice((NOTHING, SWEARS, ALL))}
            self.roster.set_clones(c, **{f: new[f] for f in fields})
            if "owner" in fields:
                st.records[c][0], st.records[c][2] = new["owner"], ALL
            if "room" in fields:
                st.records[c][1] = new["room"]
            if "hear" in fields:
                st.records[c][2] = new["hear"]
        self.seen.updated(self.label, [f"clones.{f}" for f in fields])

    def _clear_review(self, _=None) -> None:
        rooms = [self.rng.randrange(self.state.review_rooms) for _ in range(self.rng.randint(1, 2))]
        self.roster.clear_review(rooms)
        for rm in rooms:
            self.state.rings.clear(rm)
        self.seen.cleared(self.label, False)

    def _clear_revtell(self, _=None) -> None:
        slots = [self.rng.randrange(self.state.cap) for _ in range(self.rng.randint(1, 3))]
        self.roster.clear_revtell(slots)
        for j in slots:
            self.state.tell_rings.clear(j)
        self.seen.cleared(self.label, True)

    # -------------------------------------------------------------- the calls
    def _k(self, opts) -> int:
        return opts.get("k") or self.rng.randint(1, 16)

    def _text(self, opts) -> bytes:
        if "text" in opts:
            return opts["text"]
        if "sized" in opts:
            return text_of(self.rng, *opts["sized"])
        return self.rng.choice(self.pool)

    def _note(self, kind: str, timing: dict, bad: list) -> None:
        self.last_timing = timing
        self.largest = max(self.largest, timing["h2d_bytes"] + timing["d2h_bytes"])
        self.bad += [{"step": self.steps, "roster": self.label, "kind": kind, **b} for b in bad[:3]]

    def broadcasts(self, opts, relay: bool = False):
        """K ``(text, rm, sender, force_listen, com_num)`` tuples, which of them to record, and for relay_many the clone
        senders; a text to a room that holds a clone record is at most what its relay text allows."""
        rng, st = self.rng, self.state
        cloned = st.cloned_rooms() if relay else set()
        want_record = opts.get("record", rng.random() < 0.4)
        bs, record, csenders = [], [], []
        for b in range(self._k(opts)):
            rm = rng.choice((0, 0, 1, 2, 3, 4, 77, None))
            if b == 0 and opts.get("record"):
                rm = rng.randrange(st.review_rooms)
            text = self._text(opts)
            if "longest" in opts and cloned:
                rm = rng.choice(sorted(cloned))
                text = text_of(rng, 999, 999)[:longest_text(st.rooms[rm]["name"])]
            elif rm in cloned:
                text = text[:longest_text(st.rooms[rm]["name"])]
            csender = None
            if relay and rm is not None and rm < 4 and rng.random() < 0.3:
                here = [c for c, r in enumerate(st.records) if r[0] is not None and r[1] == rm]
                csender = rng.choice(here) if here else rng.randrange(st.nclones)
            sender = None if csender is not None or rng.random() < 0.3 else rng.randrange(st.cap)
            bs.append((text, rm, sender, rng.randrange(2), rng.choice(BROADCAST_COMS)))
            record.append(bool(want_record and rm is not None and rm < st.review_rooms and (rng.random() < 0.6 or (b == 0 and opts.get("record")))))
            csenders.append(csender)
        for text, *_ in bs:
            self.counts["longest_text"] = max(self.counts["longest_text"], len(text))
            self.counts["empty_texts"] += not text
        return bs, record, csenders

    def _record_broadcasts(self, bs, record) -> None:
        for (text, rm, *_), on in zip(bs, record):
            if on:
                self.state.rings.record(rm, text)
                self.counts["recorded"] += 1

    def _broadcast_many(self, opts) -> None:
        bs, _, _ = self.broadcasts(opts)
        r = self.roster.broadcast_many(bs)
        self.seen.called(self.label, "broadcast_many", False, False)
        if self.check:
            m = self.state.table_model()
            as_tables = [(t, None, int(rm is None), fl, com) for t, rm, s, fl, com in bs]
            n, first = compare(r, expected(self.cpu, as_tables, [m.records(rm, s) for _, rm, s, _, _ in bs]), as_tables)
            self._note("broadcast_many", r.timing, first[:1] if n else [])

    def _plan_many(self, opts) -> None:
        bs, record, _ = self.broadcasts(opts)
        p = self.roster.plan_many(bs, record=record if any(record) else None)
        self.seen.called(self.label, "plan_many", any(record), False)
        if self.check:
            self._note("plan_many", p.timing, plan_differences(self.cpu, p, bs, self.state.table_model()))
            self._record_broadcasts(bs, record)

    def _relay_many(self, opts) -> None:
        bs, record, csenders = self.broadcasts(opts, relay=True)
        rl = self.roster.relay_many(bs, record=record if any(record) else None,
                                    clone_sender=csenders if any(c is not None for c in csenders) else None)
        self.seen.called(self.label, "relay_many", any(record), False)
        if self.check:
            bad = plan_differences(self.cpu, rl.plan, bs, self.state.table_model())
            self._note("relay_many", rl.timing, bad + self.relay_differences(bs, csenders, rl))
            self._record_broadcasts(bs, record)

    def relay_differences(self, bs, csenders, rl: device.Relay) -> list:
        """As relay_differences of tests/device_relay_child.py, with the rooms' names from the state: the bitmap in whole
        words, the owners and their colours, the relay text and its two variants chunk by chunk."""
        st, bad = self.state, []
        records = st.relay_records()
        ignall = {j: u["ignall"] for j, u in st.users.items()}
        for k, ((text, rm, _sender, _fl, _com), cs) in enumerate(zip(bs, csenders)):
            want = relays(records, ignall, rm, cs, text)
            self.counts["relays"] += len(want)
            self.counts["clone_senders"] += cs is not None
            where = {"broadcast": k, "rm": rm, "clone_sender": cs, "text": text[:40].decode("latin-1")}
            flags = np.zeros(st.nclones, dtype=bool)
            flags[want] = True
            if rl.relay_bits[k].tolist() != device._pack(flags).tolist():
                bad.append({**where, "what": "bitmap", "device": rl.relays(k).tolist()[:20], "model": want[:20]})
                continue
            if rl.owners(k).tolist() != [records[c][0] for c in want]:
                bad.append({**where, "what": "owners"})
            if rl.owner_colours(k).tolist() != [st.users[records[c][0]]["colour"] for c in want]:
                bad.append({**where, "what": "owner colours"})
            text2 = relay_text(st.rooms[rm]["name"], text) if want else b""
            if rl.relay_text(k) != text2 or int(rl.text_sizes[k]) != (len(text2) if want else -1):
                bad.append({**where, "what": "text", "device": rl.relay_text(k)[:60].decode("latin-1")})
            for c in (0, 1):
                ch = self.cpu.chunks(text2, c) if want else []
                if rl.relay_chunks(k, c) != ch or rl.relay_variant(k, c) != b"".join(ch):
                    bad.append({**where, "what": "variant", "colour": c, "device": [len(x) for x in rl.relay_chunks(k, c)],
                                "model": [len(x) for x in ch]})
        return bad

    def _speakers(self, opts, record: bool) -> list:
        valid = self.state.speakers(ring=record)
        return [self.rng.choice(valid) for _ in range(self._k(opts))]

    def _speak_many(self, opts) -> None:
        rng, st = self.rng, self.state
        record, ban = opts.get("record", rng.random() < 0.4), rng.random() < 0.5
        events = [(j, rng.choice(SPEECH_COMS), opts["text"] if "text" in opts else text_of(rng, *opts["sized"])
                   if "sized" in opts else fuzz_inpstr(rng), rng.randrange(11)) for j in self._speakers(opts, record)]
        if opts.get("record"):                                          # a say at least: the call records
            events[0] = (events[0][0], SAY, events[0][2], events[0][3])
        recording = record and any(com in (SAY, EMOTE) for _, com, _, _ in events)
        sp = self.roster.speak_many(events, ban_swearing=ban, record=record)
        self.seen.called(self.label, "speak_many", recording, False)
        if self.check:
            self._note("speak_many", sp.timing, speech_differences(self.roster, st.users, events, ban, sp, self.counts["speech"]))
            for slot, com, inpstr, wc in events:
                m = model(st.users[slot], com, inpstr, wc, ban)
                if record and m["recorded"]:
                    st.rings.record(m["rm"], m["line"])
                    self.counts["recorded"] += 1

    def _input_many(self, opts) -> None:
        rng, st = self.rng, self.state
        record, ban = opts.get("record", rng.random() < 0.4), rng.random() < 0.5
        read = lambda: (opts["text"][:-1] + b"\n" if "text" in opts else text_of(rng, opts["sized"][0] - 1, opts["sized"][1] - 1) + b"\n"
                        if "sized" in opts else fuzz_read(rng))
        reads = [(j, read()) for j in self._speakers(opts, record)]
        inp = self.roster.input_many(reads, ban_swearing=ban, record=record)
        self.seen.called(self.label, "input_many", bool(record), False)
        if self.check:
            self._note("input_many", inp.timing, input_differences(self.roster, st.users, reads, ban, inp, self.counts["input"]))
            for slot, data in reads:
                _, m = answer_of(st.users[slot], data, ban)
                if record and m["recorded"]:
                    st.rings.record(m["rm"], m["line"])
                    self.counts["recorded"] += 1

    def _tell_many(self, opts) -> None:
        rng, st = self.rng, self.state
        record = opts.get("record", rng.random() < 0.5)
        valid = st.speakers()
        named = [j for j, u in st.users.items() if u["name"]]
        events = []
        for _ in range(self._k(opts)):
            ev = fuzz_event(rng, st.users, valid, named)
            if "text" in opts:
                ev = (ev[0], ev[1], opts["text"], 3)
            elif "sized" in opts:                                       # a word aimed at somebody, and a long rest
                word = ev[2].split(b" ")[0][:40] or b"x"
                rest = text_of(rng, *opts["sized"])
                ev = (ev[0], ev[1], (word + b" " + rest)[:len(rest)], 3)
            events.append(ev)
        pv = self.roster.tell_many(events, record=record)
        self.seen.called(self.label, "tell_many", False, bool(record))
        if self.check:
            self._note("tell_many", pv.timing, private_differences(self.roster, st.users, events, pv, self.counts["tell"]))
            for slot, com, inpstr, wc in events:
                m = private(st.users, slot, com, inpstr, wc)
                if record and m["outcome"] == TOLD:
                    st.tell_rings.record(m["target"], m["line"])
                    self.counts["told"] += 1

    def _look_many(self, opts) -> None:
        st = self.state
        seated = [j for j, u in st.users.items() if u["room"] is not None]
        slots = [self.rng.choice(seated) for _ in range(self._k(opts))]
        lk = self.roster.look_many(slots)
        self.seen.called(self.label, "look_many", False, False)
        if self.check:
            self._note("look_many", lk.timing, look_differences(st.users, st.seen_rooms(), slots, lk, self.counts["look"]))

    def _who_many(self, opts) -> None:
        """One to eight lookers, any slot at all; asked at or after every last_login."""
        rng, st = self.rng, self.state
        k = opts.get("k") or rng.randint(1, 8)
        slots = self._many([rng.randrange(st.cap) for _ in range(min(k, PERIOD))], k)
        now = NOW + rng.choice((0, 59, 60, 3600, 2**31 - 1 - NOW))
        w = self.roster.who_many(slots, now=now, date=DATE)
        self.seen.called(self.label, "who_many", False, False)
        self.counts["who_lines"] += len(listed(st.users))
        if self.check:
            bad = who_differences(st.users, st.rooms, slots[:2 * PERIOD], now, DATE, w, self.counts["who"])
            if k > 2 * PERIOD:                                          # its bitmap check wants every looker: the rest repeat
                want = np.array(bits_of(st.users, slots[:PERIOD]), dtype=np.uint32)
                bad = [b for b in bad if b["what"] != "shown"]
                if not np.array_equal(w.shown, want[np.arange(k) % PERIOD]):
                    bad.append({"what": "shown", "lookers": k})
                bad += [{"what": "a later looker", "who": i} for i in self._sample(k) if w.chunks(i) != w.chunks(i % PERIOD)]
            self._note("who_many", w.timing, bad)

    def _many(self, first: list, k: int) -> list:
        """``k`` entries that repeat ``first``: a call grown through its lookers is compared in full for the first 2 PERIOD
        of them, and for a sample of the rest with the looker it repeats."""
        return [first[i % len(first)] for i in range(k)]

    @staticmethod
    def _sample(k: int) -> list:
        return sorted(set(range(2 * PERIOD, k, max(1, k // 256))) | {k - 1})

    def _rooms_many(self, opts) -> None:
        """Lookers of both kinds in one call, or of one kind alone."""
        rng, st = self.rng, self.state
        k = self._k(opts)
        slots = self._many([rng.randrange(st.cap) for _ in range(min(k, PERIOD))], k)
        mix = rng.choice((None, None, True, False))
        kinds = self._many([rng.random() < 0.5 if mix is None else mix for _ in range(min(k, PERIOD))], k)
        got = self.roster.rooms_many(slots, topics=kinds)
        self.seen.called(self.label, "rooms_many", False, False)
        self.counts["rooms_listings"] += len(slots)
        if self.check:
            bad = rooms_differences(st.users, st.rooms, slots[:2 * PERIOD], kinds[:2 * PERIOD], got, self.counts["rooms"])
            if k > 2 * PERIOD:
                bad += [{"what": "a later looker", "looker": i} for i in self._sample(k)
                        if got.chunks(i) != got.chunks(i % PERIOD) or bool(got.topics[i]) != kinds[i]]
            self._note("rooms_many", got.timing, bad)

    def go_flags(self) -> tuple:
        """go_many's kept tables, in layout order, that the roster's flags say its next call passes."""
        r = self.roster
        flag = {"speech": r._speech_dirty, "clones": r._clones_dirty and r.clones > 0, "rooms": r._rooms_dirty, "go": r._go_dirty}
        return tuple(t for t in ("speech", "clones", "rooms", "go") if flag[t])

    def _go_events(self, opts) -> tuple:
        """The events of a go_many and the talker's two settings.  ``quiet``: nobody can move -- a word count of 1, or a
        word that begins no room's name.  ``sized``: long lines, which are quiet too.  ``returns``: slot 0, made an ARCH and
        invited there, goes out of its room, made PRIVATE, into another ring room, and too few stay behind whoever does: the
        call moves, drops an invite, returns a ring room to public and leaves its review clear pending."""
        rng, st = self.rng, self.state
        gatecrash, min_private = rng.randrange(device.MAX_LEVEL + 1), rng.randrange(4)
        if "sized" in opts:
            lo, hi = opts["sized"]
            events = [(j, (NOWHERE + b" " + text_of(rng, lo, hi))[:hi], 3) for j in self._speakers(opts, False)]
            return events, gatecrash, min_private
        if opts.get("quiet"):
            events = [(j, b"", 1) if rng.random() < 0.5 else (j, NOWHERE + rng.choice((b"", b" now")), 2)
                      for j in self._speakers(opts, False)]
            return events, gatecrash, min_private
        if opts.get("returns"):
            here = st.users[0]["room"]
            there = rng.choice([r for r in range(st.review_rooms) if r != here])
            self.renamed += 1                                           # names of one width: none begins another
            names = [b"here%04d" % self.renamed, b"there%04d" % self.renamed]
            self._put_rooms([here, there], {"name": names, "access": [device.PRIVATE, device.PUBLIC]})
            self._put_users([0], {"level": [3], "invite_room": [there]})    # the move drops the invite
            return [(0, names[1], 2)], gatecrash, st.cap + st.nclones + 1
        events = fuzz_events(rng, st.users, st.rooms, self._k(opts))      # its movers_of is State.speakers()
        # slot 0 stays in a ring room: a move of its own out of them becomes a "Go where?".  The snapshot decides as the
        # call does, because an event that an earlier one of the call could change is deferred
        for i, (slot, inpstr, wc) in enumerate(events):
            if slot == 0:
                res = go(st.users, st.rooms, st.go_clones(), slot, inpstr, wc, gatecrash, min_private)
                if res["outcome"] in MOVED and res["target"] >= st.review_rooms:
                    events[i] = (slot, inpstr, 1)
        return events, gatecrash, min_private

    def _put_rooms(self, rooms, values: dict) -> None:
        self.roster.set_rooms(rooms, **values)
        for i, rm in enumerate(rooms):
            for f in values:
                self.state.rooms[rm][f] = values[f][i]
        self.seen.updated(self.label, [f"rooms.{f}" for f in values] + ([RELAY_NAMES] if "name" in values else []))

    def _put_users(self, slots, values: dict) -> None:
        self.roster.update(slots, **values)
        for i, j in enumerate(slots):
            for f in values:
                self._took(j, f, values[f][i])
        self.seen.updated(self.label, written(values))

    def _go_many(self, opts) -> None:
        st = self.state
        events, gatecrash, min_private = self._go_events(opts)
        flags = self.go_flags()                                         # before the call, as passed() of device_kept_child.py
        invites = {j: u["invite"] for j, u in st.users.items()}
        call = go_call(st.users, st.rooms, st.go_clones(), events, gatecrash, min_private)       # the State moves
        if self.script is not None:
            self.script.append([(e["outcome"], e["target"], e["old"], int(e["returned"])) for e in call["events"]])
        got = self.roster.go_many(events, gatecrash_level=gatecrash, min_private_users=min_private)
        dropped = sum(1 for j, u in st.users.items() if u["invite"] != invites[j])
        self.seen.called(self.label, "go_many", False, False,
                         go={"moved": bool(call["movers"]), "invites_dropped": dropped, "returned": list(call["cleared"]),
                             "rings": self._rings_cleared(call["cleared"])})
        c = self.counts
        c["moves"] += len(call["movers"])
        c["returned_public"] += len(call["cleared"])
        c["deferred"] += sum(e["outcome"] == device.GO_DEFERRED for e in call["events"])
        c["invites_dropped"] += dropped
        if self.check:
            bad = go_differences(got, call, st.users, st.rooms) + mirror_differences(self.roster, st.users, st.rooms)
            self._note("go_many", got.timing, bad)
        if not self.check or not bad:
            self.seen.passed("go_many", flags)

    # -------------------------------------------------------------- the four calls that change the roster as go_many does
    def _rings_cleared(self, rooms) -> list:
        """The ring rooms among those a model's call returned to public: reset_access empties their rings."""
        rings = [rm for rm in rooms if rm < self.state.review_rooms]
        for rm in rings:
            self.state.rings.clear(rm)
        return rings

    def mirrors_differences(self) -> list:
        """The roster's mirrors against the State, after the apply step of any of the four: the rooms, the invitations and
        the rooms' access (go's comparison), the flags, descriptions, AFK messages, phrases and topics (set's), and the
        clone records where they lie (clone's)."""
        st = self.state
        return (mirror_differences(self.roster, st.users, st.rooms) + set_mirror_differences(self.roster, st.users, st.rooms)
                + record_differences(self.roster, st.go_clones()))

    def event_flags(self, kind: str, topic: bool = False) -> tuple:
        """The kept tables that the roster's flags say its next call of ``kind`` passes: go_many's four for access_many and
        clone_many; act_many's (act_flags); for set_many its own, the speaker state on any of its three flags, and the room
        table only with a ``.topic`` in the call -- without one a dirty room table is kept back."""
        if kind == "act_many":
            return self.act_flags()
        if kind != "set_many":
            return self.go_flags()
        r = self.roster
        flag = {"speech": r._speech_dirty or r._private_dirty or r._set_dirty, "afk": r._afk_dirty, "udesc": r._udesc_dirty,
                "go": r._go_dirty, "rooms": r._rooms_dirty and topic, KEPT_BACK: r._rooms_dirty and not topic}
        return tuple(t for t in SET_TABLES + (KEPT_BACK,) if flag[t])

    def _own_record(self, rm: int) -> None:
        """The Runner's own set_clones: record 0 is slot 0's, in ``rm``."""
        if self.state.records[0][:2] != [0, rm]:
            self.roster.set_clones(0, owner=0, room=rm, hear=ALL)
            self.state.records[0] = [0, rm, ALL]
            self.seen.updated(self.label, [f"clones.{f}" for f in CLONE_FIELDS])

    def _named_apart(self, rm: int, word: bytes, **more) -> bytes:
        """The Runner's own set_rooms: a name for ``rm`` that no other room's begins with, so that get_room finds it."""
        self.renamed += 1
        name = b"%s%04d" % (word, self.renamed)
        self._put_rooms([rm], {"name": [name], **{f: [v] for f, v in more.items()}})
        return name

    def _access_events(self, opts) -> tuple:
        """The events of an access_many and the talker's three settings.  ``quiet``: a word that names no room, with
        gatecrash_level 0, so that no ``.private <room>`` is refused for the level first: nothing can change.  ``sized``:
        such words with a long rest.  ``returns``: slot 0's room is made PRIVATE, some slot is invited into it, and slot 0
        says ``.public``: the call flips the access, drops the invite and leaves the room's review clear pending.
        ``invites``, for the host tier's one-by-one cases on a roster of two slots or more: slot 0's room is made PRIVATE,
        slot 1 gets a name of its own, another room and no invitation, and slot 0 invites it."""
        rng, st = self.rng, self.state
        gatecrash, min_private, ignore_mp = access_settings(rng)
        coms = (device.COM_PUBLIC, device.COM_PRIVATE, device.COM_LETMEIN)
        if "sized" in opts:
            lo, hi = opts["sized"]
            return ([(j, rng.choice(coms), (NOWHERE + b" " + text_of(rng, lo, hi))[:hi], 3) for j in self._speakers(opts, False)],
                    0, min_private, ignore_mp)
        if opts.get("quiet"):
            return ([(j, rng.choice(coms), NOWHERE + rng.choice((b"", b" now")), 2) for j in self._speakers(opts, False)],
                    0, min_private, ignore_mp)
        if opts.get("returns"):
            here = st.users[0]["room"]
            self._put_rooms([here], {"access": [device.PRIVATE]})
            self._put_users([rng.randrange(st.cap)], {"invite_room": [here]})
            return [(0, device.COM_PUBLIC, b"", 1)], gatecrash, min_private, ignore_mp
        if opts.get("invites"):
            here = st.users[0]["room"]
            self.renamed += 1
            name = b"Guest%04d" % self.renamed
            self._put_rooms([here], {"access": [device.PRIVATE]})
            self._put_users([1], {"name": [name], "login": [0], "room": [(here + 1) % LOOK_ROOMS], "invite_room": [None]})
            return [(0, device.COM_INVITE, name.lower(), 2)], gatecrash, min_private, ignore_mp
        return access_events(rng, st.users, st.rooms, self._k(opts)), gatecrash, min_private, ignore_mp

    def _access_many(self, opts) -> None:
        st, c = self.state, self.counts
        events, gatecrash, min_private, ignore_mp = self._access_events(opts)
        flags = self.event_flags("access_many")                        # before the call, as go_many's
        before = st.snapshot()
        call = access_call(st.users, st.rooms, st.go_clones(), events, gatecrash, min_private, ignore_mp)      # the State changes
        if self.script is not None:
            self.script.append([(e["outcome"], e["target_room"], e["target_slot"]) for e in call["events"]])
        got = self.roster.access_many(events, gatecrash_level=gatecrash, min_private_users=min_private, ignore_mp_level=ignore_mp)
        self.seen.called(self.label, "access_many", False, False,
                         change={"stale": st.changed_since(before), "rings": self._rings_cleared(call["cleared"])})
        outcomes = [e["outcome"] for e in call["events"]]
        c["access_effective"] += sum(o in ACCESS_EFFECTIVE for o in outcomes)
        c["access_deferred"] += outcomes.count(device.ACCESS_DEFERRED)
        c["set_private"] += outcomes.count(device.ACCESS_SET_PRIVATE)
        c["access_returned"] += len(call["cleared"])
        # the mirrors are the binding's own work: compared over a library that computes nothing too
        bad = (access_differences(got, call) if self.check else []) + self.mirrors_differences()
        self._note("access_many", got.timing, bad)
        if not bad:
            self.seen.passed("access_many", flags)

    def _clone_events(self, opts) -> tuple:
        """The events of a clone_many and the talker's three settings.  ``quiet``: a ``.csay`` or a ``.chear`` to a word that
        names no room.  ``sized``: the same with a long rest.  ``returns``: record 0 is made slot 0's in its own room, the
        room exactly PRIVATE under a name of its own, some slot invited into it, and slot 0 destroys that clone with more
        users asked for than the roster holds: the room returns to public, the records behind move down.  ``record`` True:
        the first event is a ``.csay`` of slot 0 through a record of its own, so the call has a said line to store."""
        rng, st = self.rng, self.state
        max_clones, gatecrash, min_private = clone_settings(rng)
        coms = (device.COM_CSAY, device.COM_CHEAR)
        if "sized" in opts:
            lo, hi = opts["sized"]
            return ([(j, rng.choice(coms), (NOWHERE + b" " + text_of(rng, lo, hi))[:hi], 3) for j in self._speakers(opts, False)],
                    max_clones, gatecrash, min_private)
        if opts.get("quiet"):
            rest = {device.COM_CSAY: b" hello", device.COM_CHEAR: b" all"}
            picked = [(j, rng.choice(coms)) for j in self._speakers(opts, False)]
            return [(j, com, NOWHERE + rest[com], 3) for j, com in picked], max_clones, gatecrash, min_private
        here = st.users[0]["room"]
        if opts.get("returns"):
            name = self._named_apart(here, b"den", access=device.PRIVATE)
            self._own_record(here)
            self._put_users([rng.randrange(st.cap)], {"invite_room": [here]})
            return [(0, device.COM_DESTROY, name, 2)], max_clones, gatecrash, st.cap + st.nclones + 1
        clones = st.go_clones()
        events = trim(clone_events(rng, st.users, st.rooms, clones, self._k(opts)), clones)
        if opts.get("record") and st.records_clones:
            name = self._named_apart(here, b"stage")
            self._own_record(here)
            if st.users[0]["muzzled"]:
                self._put_users([0], {"muzzled": [0]})
            events[0] = (0, device.COM_CSAY, name + b" testing, one ~OLtwo~RS", 5)
        return events, max_clones, gatecrash, min_private

    def _clone_many(self, opts) -> None:
        """``record`` is kept only on a roster whose every look room has a ring: the binding refuses it on the others."""
        st, c = self.state, self.counts
        record = bool(opts.get("record", self.rng.random() < 0.4)) and st.records_clones
        events, max_clones, gatecrash, min_private = self._clone_events(opts)
        flags = self.event_flags("clone_many")
        before = st.snapshot()
        clones = st.go_clones()
        owned_before = [i for i, r in enumerate(clones) if r is not None]
        call = clone_call(st.users, st.rooms, clones, events, max_clones, gatecrash, min_private, st.rings if record else None)
        st.take_clones(clones)                                          # moved down as the user list loses its nodes
        if self.script is not None:
            # a deferred event may have found a record that an earlier event of the call made: no index of before the call
            self.script.append([(e["outcome"], e["target_room"], e["target_slot"], e["record"] if isinstance(e["record"], int) else -1,
                                 int(e["returned"])) for e in call["events"]])
        got = self.roster.clone_many(events, max_clones=max_clones, gatecrash_level=gatecrash, min_private_users=min_private,
                                     record=record)
        self.seen.called(self.label, "clone_many", record, False,
                         change={"stale": st.changed_since(before), "rings": self._rings_cleared(call["cleared"])})
        outcomes = [e["outcome"] for e in call["events"]]
        gone = [e["record"] for e in call["events"] if e["outcome"] == device.CLONE_DESTROYED]
        c["clone_effective"] += sum(o in CLONE_EFFECTIVE for o in outcomes)
        c["clone_deferred"] += outcomes.count(device.CLONE_DEFERRED)
        c["created"] += outcomes.count(device.CLONE_CREATED)
        c["destroyed"] += len(gone)
        c["destroy_returned"] += len(call["cleared"])
        c["compacted"] += bool(gone) and any(i > min(gone) and i not in gone for i in owned_before)
        c["said_recorded"] += record * outcomes.count(device.CLONE_SAID)
        # the mirrors are the binding's own work: compared over a library that computes nothing too
        bad = (clone_differences(got, call) if self.check else []) + self.mirrors_differences()
        self._note("clone_many", got.timing, bad)
        if not bad:
            self.seen.passed("clone_many", flags)
        if st.records[0][0] is None:                                    # a .destroy took the last record: record 0 is owned
            self._set_clones(CLONE_FIELDS, at=0)

    def _set_events(self, opts) -> list:
        """The events of a set_many, by slots that have a room, a name and no login flag.  ``quiet``: queries and length
        refusals, which change nothing.  ``sized``: long descriptions, which are refused.  ``topic`` True: the first event
        is a ``.topic`` (a query in a quiet call); False: no event is one; None: as they come."""
        rng, st, G = self.rng, self.state, device
        topic = opts.get("topic")
        if "sized" in opts:
            events = [(j, G.COM_DESC, text_of(rng, *opts["sized"]), 3) for j in self._speakers(opts, False)]
        elif opts.get("quiet"):
            still = ((G.COM_DESC, b"", 1), (G.COM_INPHR, b"", 1), (G.COM_OUTPHR, b"", 1), (G.COM_DESC, b"d" * (G.USER_DESC_LEN + 1), 2),
                     (G.COM_OUTPHR, b"p" * (G.PHRASE_LEN + 1), 2), (G.COM_AFK, b"m" * (G.AFK_MESG_LEN + 1), 2))
            events = [(j, *rng.choice(still)) for j in self._speakers(opts, False)]
        else:
            events = set_events(rng, st.users, st.rooms, st.speakers(), self._k(opts))
        if topic:
            said = (b"", 1) if "sized" in opts or opts.get("quiet") else rng.choice(((b"", 1), (b"a new topic", 4), (b"t" * 60, 2), (b"~FRred/", 2)))
            events[0] = (events[0][0], G.COM_TOPIC, *said)
        elif topic is not None:
            events = [(j, G.COM_DESC, b"", 1) if com == G.COM_TOPIC else (j, com, inpstr, wc) for j, com, inpstr, wc in events]
        return events

    def _set_many(self, opts) -> None:
        st, c = self.state, self.counts
        events = self._set_events(opts)
        topic = any(com == device.COM_TOPIC for _, com, _, _ in events)
        flags = self.event_flags("set_many", topic)
        before = st.snapshot()
        call = set_call(st.users, st.rooms, events)
        for slot, *_ in events:                                         # the roster keeps afk as a flag: a locked session is AFK
            st.users[slot]["afk"] = int(bool(st.users[slot]["afk"]))
        if self.script is not None:
            self.script.append([(e["outcome"], e["reply2"] is not None) for e in call["events"]])
        got = self.roster.set_many(events)
        self.seen.called(self.label, "set_many", False, False, change={"stale": st.changed_since(before), "rings": []},
                         reads=reads_of("set_many", topic))
        outcomes = [e["outcome"] for e in call["events"]]
        c["set_effective"] += sum(o in SET_EFFECTIVE for o in outcomes)
        c["set_deferred"] += outcomes.count(device.SET_DEFERRED)
        c["topic_calls"] += topic
        c["topicless_dirty"] += KEPT_BACK in flags
        # the mirrors are the binding's own work: compared over a library that computes nothing too
        bad = (set_differences(got, call) if self.check else []) + self.mirrors_differences()
        self._note("set_many", got.timing, bad)
        if not bad:
            self.seen.passed("set_many", flags)

    def act_flags(self) -> tuple:
        """act_many's kept tables: go_many's four, but the speaker state travels after an update of ``afk`` or ``igntell``
        alone as well, since a ``.wake`` reads the target's ``afk`` bit."""
        r = self.roster
        flag = {"speech": r._speech_dirty or r._private_dirty, "clones": r._clones_dirty and r.clones > 0, "rooms": r._rooms_dirty,
                "go": r._go_dirty}
        return tuple(t for t in GO_TABLES if flag[t])

    def _act_events(self, opts) -> tuple:
        """The events of an act_many and the talker's two settings.  ``quiet``: nothing can change -- a word count of 1, or
        NOWHERE for the user, a word that no name the State draws contains, so that get_user's substring pass finds nobody.
        ``sized``: that word with a long rest.  ``returns``, on a roster of two slots or more: slot 0 is made a GOD; slot 1
        gets a name of its own, a lower level, no login flag and a ring room that is not slot 0's, made exactly PRIVATE with
        some slot invited into it, and is itself invited into slot 0's room; slot 0 moves it there with more users asked
        for than the roster holds: the call moves a user, clears both invitations, returns a ring room to public and leaves
        its review clear pending.  A roster of one slot has nobody to move, and makes an ordinary call.  ``muzzles``, for the
        host tier's one-by-one cases on a roster of two slots or more: slot 0, a GOD, muzzles slot 1, which has none.
        ``above``, likewise: slot 1 gets a GOD's muzzle through ``muzzle_level``, loses the bit and gets it back through
        ``muzzled``, which leaves the level where it was, and slot 0, a WIZ, may not remove it: ACT_UNMUZZLE_ABOVE."""
        rng, st, G = self.rng, self.state, device
        gatecrash, min_private = rng.randrange(G.MAX_LEVEL + 1), rng.randrange(4)
        coms = (G.COM_MOVE, G.COM_WAKE, G.COM_MUZZLE, G.COM_UNMUZZLE)
        if "sized" in opts:
            lo, hi = opts["sized"]
            return ([(j, rng.choice(coms), (NOWHERE + b" " + text_of(rng, lo, hi))[:hi], 3) for j in self._speakers(opts, False)],
                    gatecrash, min_private)
        if opts.get("quiet"):
            picked = [(j, rng.choice(coms)) for j in self._speakers(opts, False)]
            return ([(j, com, b"", 1) if rng.random() < 0.5 else (j, com, NOWHERE + rng.choice((b"", b" now")), 2) for j, com in picked],
                    gatecrash, min_private)
        if (opts.get("returns") or opts.get("muzzles") or opts.get("above")) and st.cap > 1:
            self.renamed += 1
            name = b"Mover%04d" % self.renamed                          # no other name contains it, and slot 0's is another
            below = rng.randrange(G.MAX_LEVEL)
            if opts.get("above"):
                self._put_users([0], {"level": [WIZ]})
                self._put_users([1], {"name": [name], "login": [0], "muzzle_level": [G.MAX_LEVEL]})
                self._put_users([1], {"muzzled": [0]})
                self._put_users([1], {"muzzled": [1]})
                return [(0, G.COM_UNMUZZLE, name.lower(), 2)], gatecrash, min_private
            self._put_users([0], {"level": [G.MAX_LEVEL]})
            if opts.get("muzzles"):
                self._put_users([1], {"name": [name], "level": [below], "login": [0], "muzzle_level": [0]})
                return [(0, G.COM_MUZZLE, name.lower(), 2)], gatecrash, min_private
            here = st.users[0]["room"]
            there = rng.choice([r for r in range(st.review_rooms) if r != here])
            self._put_rooms([there], {"access": [G.PRIVATE]})
            self._put_users([rng.choice([j for j in range(st.cap) if j != 1])], {"invite_room": [there]})
            self._put_users([1], {"name": [name], "level": [below], "login": [0], "room": [there], "invite_room": [here]})
            return [(0, G.COM_MOVE, name.lower(), 2)], gatecrash, st.cap + st.nclones + 1
        events = act_events(rng, st.users, st.rooms, self._k(opts))     # its movers_of is State.speakers()
        # slot 0 stays in a ring room: a move of it out of them becomes a usage line.  The snapshot decides as the call
        # does, because an event that an earlier one of the call could change is deferred
        for i, (slot, com, inpstr, wc) in enumerate(events):
            res = act(st.users, st.rooms, st.go_clones(), slot, com, inpstr, wc, gatecrash, min_private)
            if res["outcome"] in ACT_MOVED and res["target_slot"] == 0 and res["target_room"] >= st.review_rooms:
                events[i] = (slot, com, inpstr, 1)
        return events, gatecrash, min_private

    def _act_many(self, opts) -> None:
        st, c, G = self.state, self.counts, device
        events, gatecrash, min_private = self._act_events(opts)
        flags = self.act_flags()                                        # before the call, as go_many's
        private_alone = bool(self.roster._private_dirty and not self.roster._speech_dirty)
        before = st.snapshot()
        call = act_call(st.users, st.rooms, st.go_clones(), events, gatecrash, min_private)     # the State changes
        if self.script is not None:
            self.script.append([(e["outcome"], e["target_slot"], e["target_room"], e["old"], int(e["returned"])) for e in call["events"]])
        got = self.roster.act_many(events, gatecrash_level=gatecrash, min_private_users=min_private)
        self.seen.called(self.label, "act_many", False, False,
                         change={"stale": st.changed_since(before), "rings": self._rings_cleared(call["cleared"]),
                                 "moved": bool(call["movers"])})
        outcomes = [e["outcome"] for e in call["events"]]
        c["act_effective"] += sum(o in ACT_EFFECTIVE for o in outcomes)
        c["act_deferred"] += outcomes.count(G.ACT_DEFERRED)
        c["act_moved"] += len(call["movers"])
        c["act_returned"] += len(call["cleared"])
        c["act_invites_cleared"] += sum(1 for was, u in zip(before["invite_room"], st.users.values()) if u["invite"] != was)
        for name, outcome in (("act_muzzled", G.ACT_MUZZLED), ("act_unmuzzled", G.ACT_UNMUZZLED), ("act_woken", G.ACT_WOKEN),
                              ("act_wake_afk", G.ACT_WAKE_AFK), ("act_unmuzzle_above", G.ACT_UNMUZZLE_ABOVE)):
            c[name] += outcomes.count(outcome)
        c["act_private_alone"] += private_alone
        # the mirrors are the binding's own work: compared over a library that computes nothing too
        bad = ((act_differences(got, call, st.users) if self.check else []) + self.mirrors_differences()
               + muzzle_differences(self.roster, st.users))
        if st.users[0]["room"] is None or st.users[0]["room"] >= st.review_rooms:
            bad.append({"what": "the Runner let slot 0 be moved out of the ring rooms", "room": st.users[0]["room"]})
        self._note("act_many", got.timing, bad)
        if not bad:
            self.seen.passed("act_many", flags)

    def _review_many(self, opts) -> None:
        rooms = [self.rng.randrange(self.state.review_rooms) for _ in range(self.rng.randint(1, 4))]
        rv = self.roster.review_many(rooms)
        self.seen.called(self.label, "review_many", True, False)
        if self.check:
            self._note("review_many", rv.timing, review_differences(rv, rooms, self.state.rings, self.counts["review"], self.cache))

    def _revtell_many(self, opts) -> None:
        slots = [self.rng.randrange(self.state.cap) for _ in range(self.rng.randint(1, 8))]
        rv = self.roster.revtell_many(slots)
        self.seen.called(self.label, "revtell_many", False, True)
        if self.check:
            self._note("revtell_many", rv.timing, review_differences(rv, slots, self.state.tell_rings, self.counts["review"], self.cache))


# ------------------------------------------------------------------ the step streams
def pair_blocks() -> list:
    """[an update of one field, a call]: every kind after every field it reads, and after one it does not.  A set_many
    reads the room's topic only in a call that holds a ``.topic``: that pair forces one."""
    blocks = [[op_for(f), (kind, {"topic": True} if kind == "set_many" and f in TOPIC_READS else {})]
              for kind in KINDS for f in sorted(READS[kind])]
    return blocks + [[op_for(UNREAD[kind]), (kind, {})] for kind in KINDS]


GO_TABLES = ("speech", "clones", "rooms", "go")
#: the fields that take turns at making a kept table dirty; afk and igntell raise _private_dirty, prompt and
#: charmode_echo _set_dirty, on either of which set_many alone uploads the speaker state
SUBSET_FIELDS = {"speech": ("name", "vis", "level"), "clones": ("clones.owner", "clones.room", "clones.hear"),
                 "rooms": ("rooms.access", "rooms.links", "rooms.name", "rooms.netlink"), "go": GO_FIELDS}
#: act_many's speaker fields: afk and igntell raise _private_dirty alone, on which act_many uploads the speaker state too
ACT_SUBSET_FIELDS = {**SUBSET_FIELDS, "speech": ("name", "vis", "level", "muzzled", "muzzle_level", "afk", "igntell")}
SET_SUBSET_FIELDS = {"speech": ("name", "afk", "prompt", "vis", "igntell", "charmode_echo", "command_mode"), "afk": ("afk_mesg",),
                     "udesc": ("desc",), "go": GO_FIELDS}


def subset_blocks() -> list:
    """[a call that changes nothing and leaves its kept tables clean, an update of one field of each table of the subset,
    a call]: for go_many, access_many and clone_many every subset of their four tables is the one passed, the fields taking
    turns.  For act_many the same sixteen, the speaker state over its own fields: of the eight subsets that hold it, the
    one with the room table is reached by ``afk`` alone and the one with the room table and the go table by ``igntell``
    alone, both on ``_private_dirty``, and the one with the clone records and the go table by ``muzzle_level`` alone.  For
    set_many every subset of its first four, three times: with the room table clean, with it dirty and a ``.topic`` in the
    call, which passes it, and with it dirty and no ``.topic``, which keeps it back."""
    blocks = []
    for kind in ("go_many", "access_many", "clone_many", "act_many"):
        fields = ACT_SUBSET_FIELDS if kind == "act_many" else SUBSET_FIELDS
        for i in range(16):
            subset = [t for b, t in enumerate(GO_TABLES) if i >> b & 1]
            blocks.append([(kind, {"quiet": True})] + [op_for(fields[t][i % len(fields[t])]) for t in subset] + [(kind, {})])
    for i in range(16):
        subset = [t for b, t in enumerate(SET_TABLES[:4]) if i >> b & 1]
        dirty = [op_for(SET_SUBSET_FIELDS[t][i % len(SET_SUBSET_FIELDS[t])]) for t in subset]
        for topic in (None, True, False):
            rooms = [] if topic is None else [op_for("rooms.topic" if i % 2 else "rooms.mesg_cnt")]
            blocks.append([("set_many", {"quiet": True, "topic": True})] + dirty + rooms + [("set_many", {"topic": bool(topic)})])
    return blocks


def clear_blocks() -> list:
    """[a clear, the first call to touch those rings after it]; the clear is clear_review's, clear_revtell's, or what a
    go_many, an access_many, a clone_many or an act_many leaves that returns a ring room to public.  clone_many is among the
    first only on a roster where it may record; on the others it passes the clear by.  An act_many returns no room on a
    roster of one slot, which has nobody to move: there its block is two ordinary calls."""
    sources = [("clear_review",)] + [(kind, {"returns": True}) for kind in Coverage.CLEAR_SOURCES]
    firsts = [(kind, {"record": True}) for kind in RECORDING_KINDS + ("clone_many",)] + [("review_many", {})]
    return ([[source, first] for source in sources for first in firsts]
            + [[("clear_revtell",), ("tell_many", {"record": True})], [("clear_revtell",), ("revtell_many", {})]])


def random_op(rng: random.Random) -> tuple:
    x = rng.random()
    if x < 0.30:
        return ("update", apart(rng.sample(USER_FIELDS, rng.choice((1, 1, 2, 3, 5)))))
    if x < 0.37:
        return ("set_rooms", tuple(rng.sample(ROOM_FIELDS, rng.choice((1, 2, len(ROOM_FIELDS))))))
    if x < 0.44:
        return ("set_clones", rng.choice((("owner",), ("room",), ("hear",), CLONE_FIELDS)))
    if x < 0.48:
        return ("clear_review",)
    if x < 0.52:
        return ("clear_revtell",)
    return (rng.choice(KINDS), {})


def roster_steps(rng: random.Random, blocks: list, steps: int, each: int = 8) -> list:
    """A roster's steps: the blocks dealt to it, every clear block, an ``.unmuzzle`` of a muzzle whose bit was taken and
    put back (``above``), ``each`` calls of every kind, and random steps up to ``steps``; the blocks stay whole, their order
    is shuffled."""
    blocks = ([list(b) for b in blocks] + clear_blocks() + [[("act_many", {"above": True})]]
              + [[(kind, {})] for kind in KINDS for _ in range(each)])
    while sum(map(len, blocks)) < steps:
        blocks.append([random_op(rng)])
    rng.shuffle(blocks)
    return [op for b in blocks for op in b]


def new_roster(cap: int, nclones: int, review_rooms: int = REVIEW_ROOMS) -> device.Roster:
    return device.Roster(cap, review_rooms=review_rooms, revtell=True, look_rooms=LOOK_ROOMS, clones=nclones)


# ------------------------------------------------------------------ the parts of the device run
def sequence_part(seed: int, cov: Coverage, check: bool = True, script: list | None = None) -> dict:
    """One roster for each capacity; 1 and 64 on their own, then 65 and 257 live at once, their steps alternating; when
    the 65-slot one has made its steps it is closed and a roster of another capacity takes its handle and its turn.
    That one has a review ring for every look room, so clone_many records there and takes the pending review clears; the
    other four keep three ring rooms and the paths for rooms without a ring.
    ``check=False`` with a ``script``: over a library that computes nothing, for what the stream alone reaches."""
    rng = random.Random(seed)
    cpu = Cpu()
    pool = [t for t, _ in fuzz_items(seed, 300)] + [b"", b"x" * 999, b"\n" * 999]
    clones = (1, 65) if seed % 2 else (65, 1)
    dealt = [[] for _ in range(6)]                                      # the 257-slot roster makes twice the steps
    blocks = pair_blocks() + subset_blocks()
    rng.shuffle(blocks)
    for i, b in enumerate(blocks):
        dealt[i % 6].append(b)
    out = {"rosters": [], "n_bad": 0, "first_bad": [], "steps": 0, "counts": {}}

    def make(cap, nclones, share, steps, review_rooms=REVIEW_ROOMS):
        state = State(rng, cap, nclones, review_rooms)
        roster = new_roster(cap, nclones, review_rooms)
        state.seat(roster)
        runner = Runner(rng, roster, state, f"{seed}:{cap}/{nclones}", cov, check=check, cpu=cpu, pool=pool, script=script)
        return runner, roster_steps(rng, share, steps)

    def done(runner):
        runner.roster.close()
        out["rosters"].append({"label": runner.label, "capacity": runner.state.cap, "clones": runner.state.nclones,
                               "steps": runner.steps})
        out["n_bad"] += len(runner.bad)
        out["first_bad"] += runner.bad[:3 - len(out["first_bad"])]
        out["steps"] += runner.steps
        c = runner.counts
        for name, n in (("recorded", c["recorded"]), ("told", c["told"]), ("relays", c["relays"]), ("clone_senders", c["clone_senders"]),
                        ("empty_texts", c["empty_texts"]), ("lines_compared", c["review"]["lines_compared"]), ("moves", c["moves"]),
                        ("returned_public", c["returned_public"]), ("deferred", c["deferred"]), ("invites_dropped", c["invites_dropped"]),
                        ("who_lines", c["who_lines"]), ("rooms_listings", c["rooms_listings"]), *((name, c[name]) for name in EVENT_COUNTS)):
            out["counts"][name] = out["counts"].get(name, 0) + n
        out["counts"]["longest_text"] = max(out["counts"].get("longest_text", 0), c["longest_text"])

    for i, cap in enumerate(CAPACITIES[:2]):
        runner, steps = make(cap, clones[i % 2], dealt[i], STEPS_PER_ROSTER)
        for op in steps:
            runner.step(op)
        done(runner)
    a, a_steps = make(65, clones[0], dealt[2], STEPS_PER_ROSTER)
    b, b_steps = make(257, clones[1], dealt[3] + dealt[4], 2 * STEPS_PER_ROSTER)
    n = min(len(a_steps), len(b_steps) // 2)
    for op_a, op_b in zip(a_steps[:n], b_steps[:n]):
        a.step(op_a)
        b.step(op_b)
    for op in a_steps[n:]:
        a.step(op)
    handle = a.roster._handle                                           # mid-run: the 257-slot roster goes on
    done(a)
    c, c_steps = make(REPLACEMENT_CAPACITY, clones[1], dealt[5], STEPS_PER_ROSTER, LOOK_ROOMS)    # clone_many may record here
    rest = b_steps[n:]
    for i in range(max(len(c_steps), len(rest))):
        if i < len(c_steps):
            c.step(c_steps[i])
        if i < len(rest):
            b.step(rest[i])
    out["handle_reused"] = handle is not None and c.roster._handle == handle
    out["alternated"] = n + min(len(c_steps), len(rest))
    done(c)
    done(b)
    return out


def regrowth_part(seed: int) -> dict:
    """Every ordered pair (A, B) of the fourteen table-reading kinds on a fresh 65-slot roster whose every mirror has been
    uploaded: a tiny A, then a big B, twice.  The first B finds the allocation made anew and uploads the table from the
    pinned mirror, though the roster passes none; its repeat does not.  A big B is 16 long texts; of go_many 16 long lines
    that move nobody, or its repeat would be another call and find the table dirty; of access_many, clone_many, set_many
    and act_many for the same reason 16 long lines that change nothing (a word that names no room or no user, a description
    too long); of who_many
    and rooms_many, which take
    no text, many lookers.  A pair that does not regrow doubles K."""
    rng = random.Random(seed)
    cap, nclones = 65, 65
    state = State(rng, cap, nclones)
    cpu, cov = Cpu(), Coverage()
    tiny = {"k": 1, "text": b"hello", "record": False, "quiet": True}
    out = {"pairs": {}, "n_bad": 0, "first_bad": [], "table_slices": slice_of(4 * cap) + slice_of(cap), "with_update": 0}

    def fresh():
        roster = new_roster(cap, nclones)
        state.seat(roster)
        runner = Runner(rng, roster, state, "regrowth", cov, cpu=cpu, pool=[b"hello"])
        for kind in ("tell_many", "look_many", "relay_many", "input_many", "who_many", "go_many") + EVENT_KINDS:   # every mirror goes up once
            runner.step((kind, tiny))
        return runner

    def big(kind, k):
        return (kind, {"k": k, "sized": (900, 999), "record": False, **({"longest": True} if kind == "relay_many" else {})})

    def finish(runner):
        runner.roster.close()
        out["n_bad"] += len(runner.bad)
        out["first_bad"] += runner.bad[:3 - len(out["first_bad"])]

    for a in TABLE_KINDS:
        for b in TABLE_KINDS:
            if a == b:
                continue
            k = None
            while True:
                runner = fresh()
                runner.step((a, tiny))
                if k is None:
                    # rooms_many's allocation grows by four bytes a looker and by nothing else: it starts where the lookers
                    # alone are the most a call of this roster has copied both ways, the others at 16
                    k = max(16, runner.largest // 4 // 64 * 64) if b == "rooms_many" else 16
                state_rng = rng.getstate()
                runner.step(big(b, k))
                first = runner.last_timing["h2d_bytes"]
                rng.setstate(state_rng)                                 # the same B call once more
                runner.step(big(b, k))
                again = runner.last_timing["h2d_bytes"]
                finish(runner)
                if first != again or k >= 1 << 20:
                    break
                k *= 2
            out["pairs"][f"{a}>{b}"] = {"k": k, "first": first, "repeat": again}
            runner = fresh()                                            # Python's upload and the regrowth coincide
            runner.step((a, tiny))
            runner.step(op_for(rng.choice(TABLE_FIELDS)))
            runner.step(big(b, k))
            finish(runner)
            out["with_update"] += 1
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=SEEDS[0])
    ap.add_argument("--seed2", type=int, default=SEEDS[1])
    args = ap.parse_args()
    if device.device_count() < 1:
        print("no GPU visible", file=sys.stderr)
        return 3
    t0 = time.time()
    cov = Coverage()
    res = {"seeds": [args.seed, args.seed2], "sequence": [sequence_part(s, cov) for s in (args.seed, args.seed2)]}
    res["coverage"] = cov.as_json()
    t1 = time.time()
    res["regrowth"] = regrowth_part(args.seed + 7)
    res["seconds"] = {"sequence": round(t1 - t0, 1), "regrowth": round(time.time() - t1, 1)}
    print("DEVICE_SEQUENCE " + json.dumps(res, default=str))
    return 0


if __name__ == "__main__":
    sys.exit(main())
