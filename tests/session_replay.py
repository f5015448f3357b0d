"""One replayer for whole recorded sessions: every line step of a session of tests/golden/reference_only/replay_*.json is
answered through the calls of ``device.Roster`` and compared, client by client, with what the reference wrote.

The replayer keeps ONE state for the whole talker -- the users by slot (room, every flag, vis, level, name, desc, the two
phrases, the invite), the clone records in list order (owner, room, hear), the room table of ``session_rooms()`` (access,
topic) -- and a *backend* keeps the review and the revtell rings and answers with one method per Roster call.
``ModelBackend`` is built from the CPU models the per-call tests already pin: ``dispatch`` / ``answer_of``
(tests/device_input_child.py), ``model`` of the speech commands behind them, ``private`` and ``TellRings``
(tests/device_tell_child.py), ``look`` (tests/device_look_child.py), ``who`` (tests/device_who_child.py), ``rooms``
(tests/device_rooms_child.py), ``Rings`` (tests/device_review_child.py), ``relays`` / ``relay_text``
(tests/device_relay_child.py), ``go_call`` / ``apply_move`` (tests/device_go_child.py), ``clone_call``
(tests/device_clone_child.py), ``set_call`` / ``apply_set`` (tests/device_set_child.py), ``access_call`` / ``apply_access``
(tests/device_access_child.py) and ``nuts_path.chunks``.  ``DeviceBackend`` is one ``Roster(capacity, review_rooms=R,
revtell=True, look_rooms=R, clones=C)`` that lives for the whole session.  It is seated once, with the accounts as they
log in; after that the roster keeps its own state: what a call changes the binding has applied to the host mirrors, and the
backend uploads nothing but the clones' look-seats (below).  Both backends advance the replayer's state by the outcomes
their calls return, and after every line step the roster's host mirrors -- rooms, invites, access, every flag,
descriptions, phrases, topics, clone records -- are compared with that state.

What is taken from the recording, and nothing else, is four things: the accounts, the configuration, each step's input
line, and the bytes to compare against.  The talker's other settings (``gatecrash_level``, ``min_private``,
``ignore_mp_level``) are read from the config file ``nuts333_amd.provision`` writes.

Every line step is *answered*: every client's bytes are compared whole, the actor's included, in the reference's order.
A step's read goes through ``input_many``, and what that hands back -- ``(slot, com, inpstr, word_count)`` -- goes on as
it is to the call of its command: speech is composed by ``input_many`` itself; ``tell`` / ``pemote`` -> ``tell_many``;
``look`` -> ``look_many``; ``who`` -> ``who_many``; ``review`` -> ``review_many``; ``revtell`` -> ``revtell_many``;
``rmst`` / ``rmsn`` -> ``rooms_many``; ``go`` -> ``go_many``; ``clone``, ``destroy``, ``csay``, ``chear`` ->
``clone_many(record=True)``; ``colour``, ``ignall``, ``ignshout``, ``igntell``, ``vis``, ``invis``, ``desc``, ``topic``,
``inphr``, ``outphr`` -> ``set_many``; ``public``, ``private``, ``letmein``, ``invite`` -> ``access_many``; nothing at all
is ``Unknown command.``.  Each is a call of one event, which never defers: a ``*_DEFERRED`` outcome is a mismatch.  A line
that dispatches to anything else -- ``.afk``, ``.mode``, ``.prompt`` and ``.charecho`` among them: the return from AFK and
the prompt are the caller's -- raises ``ReplayError``; no step is skipped.

Every room line goes through two calls: the call that composed it (``input_many(record=True)``, or an event call's enter,
leave, reset, here, there or said line) and then, as a broadcast of its own, ``relay_many``, because the composing calls
leave the relay to clones' owners to the caller.  The two plans of the same line -- admit bitmap, both variants, chunk
sizes -- must be equal.  ``relay_many`` sees the roster as the event call left it, so: the enter line of a ``.go`` is
relayed with the mover as its sender (``move_user`` writes it before it moves the user, the roster has moved it); a new
clone relays the two lines of its own creation and a destroyed one nothing, as in the reference.  One line the reference
writes over a flag that ``set_many`` has already changed: ``toggle_ignall`` flips the flag behind its line
(nuts333.c:4466-4476), so that line is relayed with ``relay_many(ignall={actor: the flag as it was})``, as the two
docstrings say, and what ``relay_many`` returns is delivered as it is.  When a room returns to public -- after a ``.go``, a
``.destroy`` or a ``.public`` -- its review ring is asked for, through ``review_many``, and must be empty.

A clone is a user object in the reference's list: ``look()`` shows it, ``write_room_except`` skips it as a listener and
``get_user`` and ``who()`` pass over it.  The Roster keeps clone records apart from the slots, so the replayer also seats
every clone in a slot of its own behind the last user, in the order of the Roster's clone records -- after
``clone_many``'s compaction that is list order --, with the owner's name, the description ``~BR(CLONE)`` and the ``login``
flag: such a slot is listed by ``look_many`` and by nothing else.  A roster therefore has one slot per possible clone
behind the users' slots, and these look-seats are all that ``DeviceBackend.sync`` touches after the logins; its
``update``, ``set_clones`` and ``set_rooms`` calls are counted by slot, record and room.

``who`` is answered with ``now`` equal to every login time and ``date=b"DATE"`` (the generator masks ``long_date``), so
``mins`` is 0 in every line, as in who.json; non-zero ``mins`` stays covered by the seeded who test alone.
"""
from __future__ import annotations

import ctypes
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from device_input_child import COMMAND, SPEECH, UNKNOWN, answer_of  # noqa: E402
from device_look_child import default_rooms  # noqa: E402
from device_relay_child import relay_text, relays, swearing  # noqa: E402
from device_review_child import Rings  # noqa: E402
from device_rooms_child import list_room  # noqa: E402
from device_rooms_child import model_chunks as rooms_chunks  # noqa: E402
from device_speak_child import EMOTE, SAY, SEMOTE, SHOUT  # noqa: E402
from device_tell_child import PEMOTE, REVTELL_EMPTY, REVTELL_FOOTER, REVTELL_HEADER, TELL, TellRings, capitalised, get_user, private  # noqa: E402
from device_who_child import model_chunks as who_chunks  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402
from nuts333_amd import provision as pv  # noqa: E402

# The models of the event calls (device_go_child, device_access_child, device_clone_child, device_set_child) import this
# module for its State and its backends, so they are imported where they are used, not here.

GOLDEN = REPO / "tests" / "golden" / "reference_only"
FIRST_SEEDS = (60, 83, 155, 205, 236, 258, 267, 270)                   # the first command profile of make_replay_golden.py
SECOND_SEEDS = (8, 47, 68, 215)                                        # its second: access, rooms, desc, topic, phrases
SEEDS = FIRST_SEEDS + SECOND_SEEDS
NOW, DATE = 1000, b"DATE"
ALL, SWEARS, NOTHING = device.CLONE_HEAR_ALL, device.CLONE_HEAR_SWEARS, device.CLONE_HEAR_NOTHING
CLONE_DESC = b"~BR(CLONE)"                                              # nuts333.c:7148
NOSUCHROOM = b"There is no such room.\n"                                # nuts333.h:145
REVIEW_PRIVATE = b"That room is currently private, you cannot review the conversation.\n"   # nuts333.c:5204
REVIEW_HEADER = b"\n~BB~FG*** Review buffer for the %s ***\n\n"         # nuts333.c:5214
REVIEW_FOOTER = b"\n~BB~FG*** End ***\n\n"                              # nuts333.c:5221
REVIEW_EMPTY = b"Review buffer is empty.\n"                             # nuts333.c:5220
GO_COMMANDS = ("go",)
CLONE_COMMANDS = ("clone", "destroy", "csay", "chear")
SET_COMMANDS = ("colour", "ignall", "ignshout", "igntell", "vis", "invis", "desc", "topic", "inphr", "outphr")
ACCESS_COMMANDS = ("public", "private", "letmein", "invite")
ROOMS_COMMANDS = {"rmst": True, "rmsn": False}
ANSWERED = ("tell", "pemote", "look", "review", "revtell", "who") + GO_COMMANDS + CLONE_COMMANDS + SET_COMMANDS + ACCESS_COMMANDS + tuple(ROOMS_COMMANDS)
TRACKED = ()                                                            # every line step is answered
#: where the users sit, in login order: next to each other, or at the edges of every per-slot lane, ballot word and block
COMPACT, SPREAD = "compact", "spread"
SPREAD_SLOTS = {4: (0, 63, 64, 256), 5: (0, 63, 64, 255, 256), 6: (0, 63, 64, 128, 255, 256)}
#: the outcomes of the event calls that some session must reach, by their names in nuts333_amd.device
OUTCOMES = ("GO_WALKED", "GO_TELEPORTED", "GO_UNSEEN", "GO_NO_ROOM", "GO_ALREADY", "GO_NOT_ADJOINED", "GO_PRIVATE",
            "CLONE_CREATED", "CLONE_ALREADY", "CLONE_MAX", "CLONE_SAID", "CLONE_HEAR_ALL", "CLONE_HEAR_SWEARS", "CLONE_HEAR_NOTHING",
            "SET_COLOUR_ON", "SET_COLOUR_OFF", "SET_IGNALL_ON", "SET_IGNALL_OFF", "SET_IGNSHOUT_ON", "SET_IGNSHOUT_OFF",
            "SET_IGNTELL_ON", "SET_IGNTELL_OFF", "SET_VISIBLE", "SET_INVISIBLE",
            "ACCESS_SET_PRIVATE", "ACCESS_SET_PUBLIC", "ACCESS_INVITED", "ACCESS_ASKED", "ACCESS_TOO_FEW")
OUTCOME_NAMES = {p: {getattr(device, n): n for n in OUTCOMES if n.startswith(p)} for p in ("GO_", "CLONE_", "SET_", "ACCESS_")}
DEFERRED = {"GO_": device.GO_DEFERRED, "CLONE_": device.CLONE_DEFERRED, "SET_": device.SET_DEFERRED, "ACCESS_": device.ACCESS_DEFERRED}
COVERAGE = ("say_outside_room_0", "say_relayed", "say_withheld_by_nothing", "swears_clone_swearing", "swears_clone_clean",
            "shout_with_ignshout_listener", "tell_to_igntell", "tell_to_ignall", "tell_by_substring",
            "tell_exact_behind_substring", "line_of_200_bytes", "review_wrapped", "revtell_of_two", "line_past_clone_of_ignall_owner",
            "look_after_go_below_invisible", "who_below_invisible", "go_refused") + OUTCOMES + (
    "go_out_of_a_private_room_empties_its_ring", "go_into_an_invitation", "destroyed_with_a_notice", "compacted_record_heard",
    "look_tells_list_order_from_gap_order", "ignall_toggled_next_to_an_own_clone", "invisible_clone_created", "set_already",
    "desc_set_then_shown", "topic_set_then_shown", "phrase_set_then_walked", "access_refused", "letmein_refused", "invite_refused",
    "rmst", "rmsn")


class ReplayError(ValueError):
    """A step the replayer does not know how to answer."""


def words_of(line: bytes) -> list:
    """word[] of wordfind() over ``line``: at most ten words, each cut at 39 bytes."""
    buf = ctypes.create_string_buffer(10 * 41)
    n = nuts_path.lib().np_wordfind(line, buf)
    return [buf.raw[41 * i:41 * (i + 1)].split(b"\0", 1)[0] for i in range(n)]


def both(text):
    return None if text is None else {c: nuts_path.chunks(text, c) for c in (0, 1)}


def talker_settings() -> dict:
    """``gatecrash_level``, ``min_private`` and ``ignore_mp_level`` as provision writes them into the talker's config file."""
    init = {}
    for line in pv.TalkerConfig().render().split("ROOMS:")[0].splitlines():
        parts = line.split()
        if len(parts) == 2:
            init[parts[0]] = parts[1]
    return {"gatecrash": pv.LEVELS.index(init["gatecrash_level"]), "min_private": int(init["min_private"]),
            "ignore_mp": pv.LEVELS.index(init["ignore_mp_level"])}


def session_rooms() -> list:
    """The rooms every session was recorded with, as ``rooms()`` and ``go()`` read them: an ACCEPT room has an inlink."""
    accept = {r.name.encode() for r in pv.DEFAULT_ROOMS if r.netlink == "ACCEPT"}
    return [list_room(**{**rm, "inlink": rm["name"] in accept}) for rm in default_rooms()]


def last_word(text: bytes) -> bytes:
    """What a listing that shows ``text`` holds whatever the looker's colour: the texts the sessions set end in a plain word."""
    return text.split()[-1]


# ------------------------------------------------------------------ the state
class State:
    def __init__(self, doc: dict, layout: str):
        self.accounts = {a["name"]: a for a in doc["accounts"][0]}
        self.ban = bool(doc["config"].get("ban_swearing", False))
        self.max_clones = int(doc["config"].get("max_clones", 1))
        settings = talker_settings()
        self.gatecrash, self.min_private, self.ignore_mp = settings["gatecrash"], settings["min_private"], settings["ignore_mp"]
        self.rooms = session_rooms()
        n = len(self.accounts)
        self.seats_for = tuple(range(n)) if layout == COMPACT else SPREAD_SLOTS[n]
        self.clone_base = self.seats_for[-1] + 1
        self.clone_seats = n * self.max_clones
        self.capacity = max(8 if layout == COMPACT else 257, self.clone_base) + self.clone_seats
        self.seats, self.users, self.clones = {}, {}, []               # actor -> slot; slot -> user; [owner, room, hear]

    def login(self, actor: str, name: str) -> None:
        acc, slot = self.accounts[name], self.seats_for[len(self.seats)]
        self.seats[actor] = slot
        enc = lambda f: acc[f].encode("latin-1")
        self.users[slot] = {"slot": slot, "room": 0, "login": 0, "colour": int(bool(acc["colour"])), "ignall": 0, "ignshout": 0,
                            "igntell": 0, "vis": 1, "muzzled": int(bool(acc["muzzled"])), "level": int(acc["level"]),
                            "command_mode": int(bool(acc["command_mode"])), "name": enc("name"), "desc": enc("desc"),
                            "afk": 0, "afk_mesg": b"", "last_login": NOW, "away": None, "prompt": int(bool(acc.get("prompt", 0))),
                            "charmode_echo": int(bool(acc.get("charmode_echo", 0))), "invite": None,
                            "in_phrase": enc("in_phrase"), "out_phrase": enc("out_phrase"), "went": False}

    def everyone(self) -> dict:
        """The users and, behind them, the clones as the slots look() lists them from: record i in seat i."""
        out = dict(self.users)
        for i, c in enumerate(self.clones):
            if c is None:
                continue
            slot = self.clone_base + i
            out[slot] = {"slot": slot, "room": c[1], "login": 1, "colour": 0, "ignall": 0, "ignshout": 0, "igntell": 0, "vis": 1,
                         "muzzled": 0, "level": 0, "command_mode": 0, "name": self.users[c[0]]["name"], "desc": CLONE_DESC,
                         "afk": 0, "afk_mesg": b"", "last_login": NOW, "away": None, "prompt": 0, "charmode_echo": 0, "invite": None,
                         "in_phrase": b"enters", "out_phrase": b"goes"}
        return out

    def records(self) -> list:
        """The clone records as relays() reads them; the list has no empty record unless a model left one."""
        return [(None, None, None) if c is None else tuple(c) for c in self.clones]

    def table(self) -> list:
        """The records as the event calls' models read them: one entry per record of the roster, None where it is empty."""
        return [None if c is None else tuple(c) for c in self.clones] + [None] * (self.clone_seats - len(self.clones))

    def get_room(self, word: bytes):
        return next((i for i, r in enumerate(self.rooms) if r["name"].startswith(word)), None)       # nuts333.c:2388-2389

    def has_room_access(self, u: dict, rm: int) -> bool:                # nuts333.c:2416-2420
        import device_go_child
        return device_go_child.has_room_access(u, self.rooms, rm, self.gatecrash)

    def find_clone(self, owner: int, rm):
        return next((i for i, c in enumerate(self.clones) if c is not None and c[0] == owner and c[1] == rm), None)


# ------------------------------------------------------------------ the backends
def answer(outcome: int, texts: dict, plans: dict, **more) -> dict:
    """What an event call's method hands to the replayer, from either backend."""
    return {"outcome": outcome, "texts": texts, "plans": plans, "target_room": -1, "target_slot": -1, "record": -1, "returned": False,
            "look": None, **more}


class ModelBackend:
    """One method per Roster call, from the CPU models of the per-call tests."""

    def __init__(self, st: State):
        self.st = st
        self.rings, self.tells = Rings(len(st.rooms)), TellRings(st.capacity)

    def sync(self) -> None:
        self.all = self.st.everyone()

    def close(self) -> None:
        pass

    def mirror(self) -> list:
        return []

    def _plan(self, text: bytes, rm, sender, force_listen: int, com: int, ignall=None) -> dict:
        admitted = [j for j, u in sorted(self.all.items())
                    if nuts_path.admits([u["login"], int(u["room"] is not None), int(rm is not None and u["room"] == rm),
                                         u["ignall"] if ignall is None else ignall[j],
                                         u["ignshout"], int(j == sender)], int(rm is None), force_listen, com)]
        return {"admitted": admitted, "chunks": both(text), "bits": None}

    def _answer(self, res: dict, kinds, **more) -> dict:
        return answer(res["outcome"], {kind: res[kind] for kind in kinds},
                      {kind: {"admitted": res["plans"][kind], "chunks": both(res[kind]), "bits": None} for kind in kinds}, **more)

    def input(self, slot: int, data: bytes, record: bool) -> dict:
        d, m = answer_of(self.all[slot], data, self.st.ban)
        if record and m["recorded"]:
            self.rings.record(m["rm"], m["line"])
        return {"kind": d["kind"], "com": d["com"], "word_count": d["word_count"],
                "inpstr": data[d["start"]:d["start"] + d["size"]] if d["size"] >= 0 else b"", "reply": both(m["reply"]),
                "line": m["line"], "plan": None if m["line"] is None else self._plan(m["line"], m["rm"], m["sender"], 0, d["com"])}

    def relay(self, broadcasts, record=None, clone_sender=None, ignall=None) -> list:
        out = []
        flags = {**{j: u["ignall"] for j, u in self.all.items()}, **(ignall or {})}     # relay_many(ignall=): the flags as given
        for k, (text, rm, sender, fl, com) in enumerate(broadcasts):
            cs = clone_sender[k] if clone_sender else None
            who = relays(self.st.records(), flags, rm, cs, text)
            ch = both(relay_text(self.st.rooms[rm]["name"], text)) if who else None
            out.append({"plan": self._plan(text, rm, sender, fl, com, flags), "relays": [(self.st.clones[c][0], ch) for c in who]})
            if record and record[k]:
                self.rings.record(rm, text)
        return out

    def tell(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        m = private(self.all, slot, com, inpstr, word_count)
        if m["line"] is not None:
            self.tells.record(m["target"], m["line"])
        return {"reply": both(m["reply"]), "line": both(m["line"]), "target": m["target"]}

    def look(self, slot: int) -> bytes:
        import device_go_child
        return b"".join(device_go_child.look_of(self.all, self.st.rooms, slot))

    def who(self, slot: int) -> bytes:
        return b"".join(who_chunks(self.all, self.st.rooms, slot, NOW, DATE))

    def rooms(self, slot: int, topics: bool) -> bytes:
        return b"".join(rooms_chunks(self.all, self.st.rooms, slot, topics))

    def review(self, rm: int) -> dict:
        return {"lines": len(self.rings.lines(rm)), **{c: self.rings.chunks(rm, c) for c in (0, 1)}}

    def revtell(self, slot: int) -> dict:
        return {"lines": len(self.tells.lines(slot)), **{c: self.tells.chunks(slot, c) for c in (0, 1)}}

    # -- the event calls: one event through the model, which changes the users, the rooms and the records as the event does
    def go(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        import device_go_child as g
        st = self.st
        call = g.go_call(self.all, st.rooms, st.table(), [(slot, inpstr, word_count)], st.gatecrash, st.min_private)
        res = call["events"][0]
        for rm in call["cleared"]:
            self.rings.clear(rm)
        return self._answer(res, ("enter", "leave", "reset", "reply"), room=res["old"], target_room=res["target"], returned=res["returned"],
                            look=b"".join(res["look"]) if res["outcome"] in g.MOVED else None)

    def clone(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        import device_clone_child as c
        st = self.st
        table = st.table()
        call = c.clone_call(self.all, st.rooms, table, [(slot, com, inpstr, word_count)], st.max_clones, st.gatecrash, st.min_private,
                            self.rings)
        while table and table[-1] is None:
            table.pop()
        st.clones = [None if rec is None else list(rec) for rec in table]
        res = call["events"][0]
        return self._answer(res, c.KINDS, room=res["room"], target_room=res["target_room"], target_slot=res["target_slot"],
                            record=res["record"], returned=res["returned"])

    def set(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        import device_set_child as s
        res = s.set_call(self.all, self.st.rooms, [(slot, com, inpstr, word_count)])["events"][0]
        return self._answer(res, s.KINDS, room=res["room"], reply_colour=res["reply_colour"])

    def access(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        import device_access_child as a
        st = self.st
        call = a.access_call(self.all, st.rooms, st.table(), [(slot, com, inpstr, word_count)], st.gatecrash, st.min_private, st.ignore_mp)
        res = call["events"][0]
        for rm in call["cleared"]:
            self.rings.clear(rm)
        return self._answer(res, a.KINDS, room=res["room"], target_room=res["target_room"], target_slot=res["target_slot"])


USER_FIELDS = ("room", "login", "colour", "ignall", "ignshout", "igntell", "vis", "muzzled", "level", "command_mode", "name",
               "desc", "last_login")
LOGIN_FIELDS = ("afk", "afk_mesg", "in_phrase", "out_phrase", "prompt", "charmode_echo")


class DeviceBackend:
    """The same methods over one Roster that lives for the session.  ``sync`` seats an account when it has logged in and,
    after that, the clones' look-seats alone: everything else the calls own, and the binding has applied it to the mirrors.
    ``uploads`` counts the ``update``, ``set_clones`` and ``set_rooms`` calls made after a slot's login, by what they address."""

    def __init__(self, st: State):
        import device_go_child
        self.st = st
        r = len(st.rooms)
        self.roster = device.Roster(st.capacity, review_rooms=r, revtell=True, look_rooms=r, clones=st.clone_seats)
        device_go_child.set_rooms(self.roster, st.rooms)
        self.sent, self.sent_clones = {}, [None] * st.clone_seats
        self.calls, self.uploads = {}, {"update": {}, "set_clones": {}, "set_rooms": {}}

    def close(self) -> None:
        self.roster.close()

    def _count(self, what: str) -> None:
        self.calls[what] = self.calls.get(what, 0) + 1

    def _upload(self, kind: str, at: int, seating: bool = False, **fields) -> None:
        """Every write of the backend's into the roster: ``kind`` is update, set_clones or set_rooms."""
        getattr(self.roster, kind)(at, **fields)
        if not seating:
            self.uploads[kind][at] = self.uploads[kind].get(at, 0) + 1

    def sync(self) -> None:
        now = self.st.everyone()
        for slot in sorted(set(now) | set(self.sent)):
            if slot in self.st.users:
                if slot not in self.sent:                               # the login, and nothing after it
                    u = now[slot]
                    self.sent[slot] = {f: u[f] for f in USER_FIELDS}
                    self._upload("update", slot, seating=True, **self.sent[slot], invite_room=u["invite"], **{f: u[f] for f in LOGIN_FIELDS})
                continue
            want = ({f: now[slot][f] for f in USER_FIELDS} if slot in now
                    else {**self.sent[slot], "room": None, "login": 1})             # a clone's seat after its .destroy
            changed = {f: v for f, v in want.items() if slot not in self.sent or self.sent[slot][f] != v}
            if changed:
                self._upload("update", slot, **changed)
                self.sent[slot] = want

    def mirror(self) -> list:
        """The roster's host mirrors against the replayer's state: what the binding applied, and nobody uploaded."""
        import device_clone_child
        import device_go_child
        import device_set_child
        st = self.st
        return (device_go_child.mirror_differences(self.roster, st.users, st.rooms)
                + device_set_child.mirror_differences(self.roster, st.users, st.rooms)
                + device_clone_child.record_differences(self.roster, st.table()))

    def _plan(self, plan: device.Plan, k: int) -> dict:
        return {"admitted": np.flatnonzero(plan.admitted(k)).tolist(), "chunks": {c: plan.chunks(k, c) for c in (0, 1)},
                "bits": plan.admitted_bits[k].tobytes() + b"".join(plan.variant(k, c) for c in (0, 1))}

    def _answer(self, got, kinds, **more) -> dict:
        return answer(int(got.outcome[0]), {kind: text(0) if got.text_sizes[row, 0] >= 0 else None for row, (kind, _, text) in enumerate(kinds)},
                      {kind: self._plan(plan, 0) for kind, plan, _ in kinds}, **more)

    def input(self, slot: int, data: bytes, record: bool) -> dict:
        inp = self.roster.input_many([(slot, data)], ban_swearing=self.st.ban, record=record)
        self._count("input_many")
        sp = inp.speech
        return {"kind": int(inp.kind[0]), "com": int(inp.com[0]), "word_count": int(inp.word_count[0]), "inpstr": inp.inpstr(0),
                "reply": {c: sp.reply.chunks(0, c) for c in (0, 1)} if sp.reply_text(0) else None,
                "line": sp.line(0) or None, "plan": self._plan(sp.room, 0) if sp.line(0) else None}

    def relay(self, broadcasts, record=None, clone_sender=None, ignall=None) -> list:
        rl = self.roster.relay_many(broadcasts, record=record, clone_sender=clone_sender, ignall=ignall)
        self._count("relay_many")
        out = []
        for k in range(len(broadcasts)):
            ch = {c: rl.relay_chunks(k, c) for c in (0, 1)}
            out.append({"plan": self._plan(rl.plan, k), "relays": [(int(o), ch) for o in rl.owners(k)]})
        return out

    def tell(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        pv_ = self.roster.tell_many([(slot, com, inpstr, word_count)], record=True)
        self._count("tell_many")
        target = int(pv_.target[0])
        return {"reply": {c: pv_.reply.chunks(0, c) for c in (0, 1)},
                "line": {c: pv_.told.chunks(0, c) for c in (0, 1)} if pv_.line(0) else None, "target": None if target < 0 else target}

    def look(self, slot: int) -> bytes:
        self._count("look_many")
        return self.roster.look_many([slot]).output(0)

    def who(self, slot: int) -> bytes:
        self._count("who_many")
        return self.roster.who_many([slot], now=NOW, date=DATE).output(0)

    def rooms(self, slot: int, topics: bool) -> bytes:
        self._count("rooms_many")
        return self.roster.rooms_many([slot], topics=topics).output(0)

    def review(self, rm: int) -> dict:
        self._count("review_many")
        rv = self.roster.review_many([rm])
        return {"lines": int(rv.line_counts[0]), **{c: rv.chunks(0, c) for c in (0, 1)}}

    def revtell(self, slot: int) -> dict:
        self._count("revtell_many")
        rv = self.roster.revtell_many([slot])
        return {"lines": int(rv.line_counts[0]), **{c: rv.chunks(0, c) for c in (0, 1)}}

    # -- the event calls: one event a call, with the session's settings.  The binding has applied the event to the roster's
    # mirrors; the replayer's state takes the same change from what the call returned, and nothing of it is uploaded
    def go(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        import device_go_child as g
        st = self.st
        got = self.roster.go_many([(slot, inpstr, word_count)], gatecrash_level=st.gatecrash, min_private_users=st.min_private)
        self._count("go_many")
        a = self._answer(got, g.texts_of(got), room=int(got.old_room[0]), target_room=int(got.target[0]), returned=bool(got.returned_public[0]))
        if a["outcome"] in g.MOVED:
            g.apply_move(st.users, st.rooms, {"slot": slot, "target": a["target_room"], "old": a["room"], "returned": a["returned"],
                                              "look": None}, [])
            a["look"] = got.look.output(0)
        return a

    def clone(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        import device_clone_child as c
        st = self.st
        got = self.roster.clone_many([(slot, com, inpstr, word_count)], max_clones=st.max_clones, gatecrash_level=st.gatecrash,
                                     min_private_users=st.min_private, record=True)
        self._count("clone_many")
        a = self._answer(got, c.texts_of(got), room=st.users[slot]["room"], target_room=int(got.target_room[0]),
                         target_slot=int(got.target_slot[0]), record=int(got.record[0]), returned=bool(got.reset[0]))
        if a["outcome"] <= device.CLONE_HEAR_ALL:
            st.clones[a["record"]][2] = a["outcome"]
        elif a["outcome"] == device.CLONE_CREATED:
            st.clones.append([slot, a["target_room"], ALL])
        elif a["outcome"] == device.CLONE_DESTROYED:
            del st.clones[a["record"]]                                  # the later records move down
            if a["returned"]:                                           # reset_access, c:2097-2104
                st.rooms[a["target_room"]]["access"] = device.PUBLIC
                for u in st.users.values():
                    if u["invite"] == a["target_room"]:
                        u["invite"] = None
        return a

    def set(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        import device_set_child as s
        st = self.st
        model = s.setting(st.users, st.rooms, slot, com, inpstr, word_count)   # for what an effective event changes, no more
        got = self.roster.set_many([(slot, com, inpstr, word_count)])
        self._count("set_many")
        a = self._answer(got, s.texts_of(got), room=st.users[slot]["room"], reply_colour=int(got.reply_colour[0]))
        if a["outcome"] in s.EFFECTIVE and a["outcome"] == model["outcome"]:
            s.apply_set(st.users, st.rooms, model)
        return a

    def access(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        import device_access_child as ac
        st = self.st
        got = self.roster.access_many([(slot, com, inpstr, word_count)], gatecrash_level=st.gatecrash, min_private_users=st.min_private,
                                      ignore_mp_level=st.ignore_mp)
        self._count("access_many")
        a = self._answer(got, ac.texts_of(got), room=st.users[slot]["room"], target_room=int(got.target_room[0]),
                         target_slot=int(got.target_slot[0]))
        if a["outcome"] in ac.EFFECTIVE:
            ac.apply_access(st.users, st.rooms, a, [])
        return a


class UploadingBackend(DeviceBackend):
    """A roster that is told the replayer's state: ``sync`` uploads every field that changed since the last step, the users'
    too.  For the replayers of the per-call tests, whose sessions hold commands that change the state and go through no
    call; comparing such a roster's mirrors with the state it was given says nothing."""

    def sync(self) -> None:
        now = self.st.everyone()
        for slot in sorted(set(now) | set(self.sent)):
            want = ({f: now[slot][f] for f in USER_FIELDS} if slot in now
                    else {**self.sent[slot], "room": None, "login": 1})             # a clone's slot after its .destroy
            changed = {f: v for f, v in want.items() if slot not in self.sent or self.sent[slot][f] != v}
            if changed:
                self._upload("update", slot, **changed)
                self.sent[slot] = want
        records = self.st.table()
        for c, rec in enumerate(records):
            if rec != self.sent_clones[c]:
                if rec is None:
                    self._upload("set_clones", c, owner=None)
                else:
                    self._upload("set_clones", c, owner=rec[0], room=rec[1], hear=rec[2])
                self.sent_clones[c] = rec

    def mirror(self) -> list:
        return []


# ------------------------------------------------------------------ the replayer
class Replayer:
    def __init__(self, doc: dict, backend_class=ModelBackend, layout: str = COMPACT, everyone_in_room_0: bool = False):
        self._begin(doc, State(doc, layout), backend_class)
        self.frozen = everyone_in_room_0            # the old replay_reads assumption, kept to show that it now fails

    def _begin(self, doc: dict, st: State, backend_class) -> None:
        """What every replayer starts from, the per-call tests' with a State of their own."""
        self.doc, self.st = doc, st
        self.backend = backend_class(st)
        self.frozen = False
        self.recorded = {}                          # room -> lines recorded into its ring since it was last emptied
        self.res = {"answered": 0, "tracked": 0, "comparisons": 0, "plan_checks": 0, "plan_disagreements": 0, "mismatches": [],
                    "commands": {}, "coverage": {k: 0 for k in COVERAGE}, "capacity": st.capacity, "slots": [], "mirror_checks": 0}
        # what the coverage counts remember between steps: the (owner, room) of the records that moved down behind a
        # destroyed one, the same records in a table whose gaps a new clone fills, and the texts set and not yet shown
        self.notes = {"moved": set(), "gappy": [], "desc": {}, "topic": {}, "phrase": set()}

    # -- delivery
    def _deliver(self, out: dict, parts: list) -> None:
        """``parts`` is what relay() returns: the direct line to every admitted user, then every relay to its owner."""
        users = self.st.users
        for p in parts:
            for j in p["plan"]["admitted"]:
                if j in users:
                    out[j] += b"".join(p["plan"]["chunks"][users[j]["colour"]])
            for owner, ch in p["relays"]:
                out[owner] += b"".join(ch[users[owner]["colour"]])

    def _broadcast(self, out: dict, broadcasts, record=None, clone_sender=None) -> list:
        """Lines the caller composed itself, through relay_many: what the replayers of the per-call tests write of theirs."""
        self.backend.sync()
        parts = self.backend.relay(broadcasts, record=record, clone_sender=clone_sender)
        self._deliver(out, parts)
        for k, (text, rm, _s, _f, com) in enumerate(broadcasts):
            if record and record[k]:
                self._note_record(rm, text)
            self._note_clones(rm, text, parts[k], com)
        return parts

    def _note_record(self, rm: int, text: bytes) -> None:
        self.recorded[rm] = self.recorded.get(rm, 0) + 1
        self.res["coverage"]["line_of_200_bytes"] += len(text) >= 200

    def _note_clones(self, rm, text: bytes, part: dict, com: int) -> None:
        cov, users = self.res["coverage"], self.st.users
        clones = [c for c in self.st.clones if c is not None]
        here = [c for c in clones if c[1] == rm and not users[c[0]]["ignall"]]
        if com == SAY:
            cov["say_relayed"] += bool(part["relays"])
            cov["say_withheld_by_nothing"] += any(c[2] == NOTHING for c in here)
        cov["line_past_clone_of_ignall_owner"] += any(c[1] == rm and users[c[0]]["ignall"] and (c[2] == ALL or c[2] == SWEARS and swearing(text))
                                                      for c in clones)
        if any(c[2] == SWEARS for c in here):
            cov["swears_clone_swearing" if swearing(text) else "swears_clone_clean"] += 1
        cov["compacted_record_heard"] += any((owner, rm) in self.notes["moved"] for owner, _ in part["relays"])

    def _room_line(self, out: dict, a: dict, kind: str, rm: int, sender, com: int, ignall=None) -> None:
        """A room line an event call composed and planned: through relay_many as a broadcast of its own, whose plan of it
        must be the call's; delivered by the call's plan and relay_many's relays."""
        text = a["texts"][kind]
        if text is None:
            return
        part = self.backend.relay([(text, rm, sender, 0, com)], ignall=ignall)[0]
        self.res["plan_checks"] += 1
        if part["plan"] != a["plans"][kind]:
            self.res["plan_disagreements"] += 1
        part = {"plan": a["plans"][kind], "relays": part["relays"]}
        self._deliver(out, [part])
        self._note_clones(rm, text, part, com)

    def _returned_to_public(self, index: int, step: dict, rm: int) -> None:
        """reset_access and ``.public`` empty the room's review buffer (c:2104, 4611): the backend's ring is asked for."""
        self.recorded[rm] = 0
        lines = self.backend.review(rm)["lines"]
        if lines:
            self.res["mismatches"].append({"step": index, "send": step["send"][:80], "what": f"room {rm} returned to public with {lines} lines in its ring"})

    def _outcome(self, index: int, step: dict, call: str, outcome: int) -> None:
        name = OUTCOME_NAMES[call].get(outcome)
        if name:
            self.res["coverage"][name] += 1
        if outcome == DEFERRED[call]:
            self.res["mismatches"].append({"step": index, "send": step["send"][:80], "what": f"a call of one event deferred ({call}DEFERRED)"})

    # -- the commands
    def _speech(self, u: dict, inp: dict, out: dict) -> None:
        cov, users = self.res["coverage"], self.st.users
        if inp["reply"] is not None:
            out[u["slot"]] += b"".join(inp["reply"][u["colour"]])
        if inp["line"] is None:
            return
        com = inp["com"]
        rm = u["room"] if com in (SAY, EMOTE) else None                 # nuts333.c:4098, 4204; 4123, 4225
        sender = u["slot"] if com in (SAY, SHOUT) else None             # write_room_except(.., user); write_room(..)
        if com in (SAY, EMOTE):                                         # record(user->room, text), nuts333.c:4099, 4205
            self._note_record(rm, inp["line"])
        part = self.backend.relay([(inp["line"], rm, sender, 0, com)])[0]
        self.res["plan_checks"] += 1
        if part["plan"] != inp["plan"]:
            self.res["plan_disagreements"] += 1
        self._deliver(out, [{"plan": inp["plan"], "relays": part["relays"]}])
        self._note_clones(rm, inp["line"], part, com)
        heard = [j for j in inp["plan"]["admitted"] if j in users]
        cov["say_outside_room_0"] += com == SAY and rm != 0 and bool(heard)
        cov["shout_with_ignshout_listener"] += com == SHOUT and any(x["ignshout"] for j, x in users.items() if j != u["slot"])

    def _tell(self, u: dict, inp: dict, out: dict) -> None:
        cov, users = self.res["coverage"], self.st.users
        t = self.backend.tell(u["slot"], inp["com"], inp["inpstr"], inp["word_count"])
        out[u["slot"]] += b"".join(t["reply"][u["colour"]])
        if t["line"] is not None:
            out[t["target"]] += b"".join(t["line"][users[t["target"]]["colour"]])
        if t["target"] is not None and t["target"] in users:
            who, word = users[t["target"]], capitalised(words_of(inp["inpstr"])[0])
            cov["tell_to_igntell"] += bool(who["igntell"])
            cov["tell_to_ignall"] += bool(who["ignall"])
            cov["tell_by_substring"] += word in who["name"] and not who["name"].startswith(word)
            cov["tell_exact_behind_substring"] += word == who["name"] and any(word in x["name"] for j, x in users.items() if j < who["slot"])

    def _review(self, u: dict, inp: dict) -> bytes:
        c, rm = u["colour"], u["room"]
        if inp["word_count"] >= 2:                                      # nuts333.c:5198-5207
            rm = self.st.get_room(words_of(inp["inpstr"])[0])
            if rm is None:
                return nuts_path.transduce(NOSUCHROOM, c)
            if not self.st.has_room_access(u, rm):
                return nuts_path.transduce(REVIEW_PRIVATE, c)
        rv = self.backend.review(rm)
        self.res["coverage"]["review_wrapped"] += self.recorded.get(rm, 0) > device.REVIEW_LINES and rv["lines"] == device.REVIEW_LINES
        if not rv["lines"]:
            return nuts_path.transduce(REVIEW_EMPTY, c)
        return (nuts_path.transduce(REVIEW_HEADER % self.st.rooms[rm]["name"], c) + b"".join(rv[c])
                + nuts_path.transduce(REVIEW_FOOTER, c))

    def _revtell(self, u: dict) -> bytes:
        c = u["colour"]
        rv = self.backend.revtell(u["slot"])
        self.res["coverage"]["revtell_of_two"] += rv["lines"] >= 2
        if not rv["lines"]:
            return nuts_path.transduce(REVTELL_EMPTY, c)
        return nuts_path.transduce(REVTELL_HEADER, c) + b"".join(rv[c]) + nuts_path.transduce(REVTELL_FOOTER, c)

    def _below_invisible(self, u: dict, same_room: bool) -> bool:
        return any(not x["vis"] and x["level"] > u["level"] and (not same_room or x["room"] == u["room"])
                   for j, x in self.st.users.items() if j != u["slot"])

    def _shown(self, what: str, holders, listing: bytes) -> None:
        """Counts a text set earlier -- ``what`` is desc or topic, ``holders`` whose the listing could show -- that it shows."""
        fresh = self.notes[what]
        for key in [k for k in holders if k in fresh and last_word(fresh[k]) in listing]:
            self.res["coverage"][what + "_set_then_shown"] += 1
            del fresh[key]

    def _look(self, u: dict, out: dict) -> None:
        st, cov, notes = self.st, self.res["coverage"], self.notes
        cov["look_after_go_below_invisible"] += u["went"] and self._below_invisible(u, True)
        here = lambda table: [c[0] for c in table if c is not None and c[1] == u["room"]]
        cov["look_tells_list_order_from_gap_order"] += here(st.clones) != here(notes["gappy"])
        listing = self.backend.look(u["slot"])
        self._shown("desc", [j for j, x in st.users.items() if j != u["slot"] and x["room"] == u["room"]], listing)
        self._shown("topic", [u["room"]], listing)
        out[u["slot"]] += listing

    def _go(self, index: int, step: dict, u: dict, inp: dict, out: dict) -> None:
        """go() and move_user() (c:4384-4457): the enter line, the leave line, the look, what reset_access writes, or the refusal."""
        cov, slot, com, notes = self.res["coverage"], u["slot"], inp["com"], self.notes
        invited, in_ring = u["invite"], self.recorded.get(u["room"], 0)
        a = self.backend.go(slot, com, inp["inpstr"], inp["word_count"])
        self._outcome(index, step, "GO_", a["outcome"])
        if a["outcome"] == device.GO_NETLINK:
            raise ReplayError(f"step {index}: {step['send']!r} goes over a netlink, which is the caller's")
        moved = a["look"] is not None
        cov["go_refused"] += not moved and inp["word_count"] >= 2
        if moved:
            u["went"] = True
            cov["go_into_an_invitation"] += invited == a["target_room"]
            cov["phrase_set_then_walked"] += a["outcome"] == device.GO_WALKED and slot in notes["phrase"]
            if self.frozen:
                u["room"] = a["room"]
        # move_user writes the enter line before it moves the user; the roster has moved it, so the mover is the sender
        self._room_line(out, a, "enter", a["target_room"], slot, com)
        self._room_line(out, a, "leave", a["room"], slot, com)
        if moved:
            out[slot] += a["look"]
        if a["returned"]:
            cov["go_out_of_a_private_room_empties_its_ring"] += in_ring > 0
            self._returned_to_public(index, step, a["room"])
        self._room_line(out, a, "reset", a["room"], slot, com)
        if a["texts"]["reply"] is not None:
            out[slot] += b"".join(a["plans"]["reply"]["chunks"][u["colour"]])

    def _clone(self, index: int, step: dict, u: dict, inp: dict, out: dict) -> None:
        """create_clone, destroy_clone, clone_say and clone_hear (c:7109-7205, 7300-7356), in their order of writing."""
        st, cov, slot, com, notes = self.st, self.res["coverage"], u["slot"], inp["com"], self.notes
        before = [None if c is None else (c[0], c[1]) for c in st.clones]
        a = self.backend.clone(slot, com, inp["inpstr"], inp["word_count"])
        self._outcome(index, step, "CLONE_", a["outcome"])
        self.backend.sync()                                             # the clones' seats, for the looks that follow
        rm = a["target_room"]
        if a["outcome"] == device.CLONE_CREATED:
            if None in notes["gappy"]:
                notes["gappy"][notes["gappy"].index(None)] = (slot, rm)
            else:
                notes["gappy"].append((slot, rm))
            cov["invisible_clone_created"] += not u["vis"]
        elif a["outcome"] == device.CLONE_DESTROYED:
            gone = before[a["record"]]
            notes["moved"] = (notes["moved"] | {rec for rec in before[a["record"] + 1:] if rec is not None}) - {gone}
            if gone in notes["gappy"]:                                  # not a record that another replayer's .switch moved
                notes["gappy"][notes["gappy"].index(gone)] = None
            cov["destroyed_with_a_notice"] += a["texts"]["notice"] is not None
        elif a["outcome"] == device.CLONE_SAID:
            cov["compacted_record_heard"] += (slot, rm) in notes["moved"]
        if a["returned"]:
            self._returned_to_public(index, step, rm)
        self._room_line(out, a, "reset", rm, None, com)                 # reset_access runs before anything is written
        if a["texts"]["reply"] is not None:
            out[slot] += b"".join(a["plans"]["reply"]["chunks"][u["colour"]])
        self._room_line(out, a, "here", a["room"], slot, com)
        self._room_line(out, a, "there", rm, slot if a["outcome"] == device.CLONE_CREATED else None, com)
        if a["texts"]["notice"] is not None:
            who = a["target_slot"]
            out[who] += b"".join(a["plans"]["notice"]["chunks"][st.users[who]["colour"]])
        if a["texts"]["said"] is not None:
            self._note_record(rm, a["texts"]["said"])
        self._room_line(out, a, "said", rm, None, com)

    def _set(self, index: int, step: dict, u: dict, inp: dict, out: dict) -> None:
        """The commands a user sets its own state with: the replies, then the here line."""
        st, cov, slot, com, notes = self.st, self.res["coverage"], u["slot"], inp["com"], self.notes
        colour = u["colour"]
        a = self.backend.set(slot, com, inp["inpstr"], inp["word_count"])
        self._outcome(index, step, "SET_", a["outcome"])
        if a["outcome"] == device.SET_COLOUR_TEST:                      # the caller's: twenty write_user calls
            out[slot] += b"".join(nuts_path.transduce(line, colour) for line in device.COLOUR_TEST)
        for kind in ("reply", "reply2"):
            if a["texts"][kind] is not None:
                out[slot] += b"".join(a["plans"][kind]["chunks"][a["reply_colour"]])
        as_it_was = None
        if a["outcome"] in (device.SET_IGNALL_ON, device.SET_IGNALL_OFF):      # toggle_ignall flips the flag behind its line
            as_it_was = {slot: int(a["outcome"] == device.SET_IGNALL_OFF)}
            cov["ignall_toggled_next_to_an_own_clone"] += any(c is not None and c[0] == slot and c[1] == a["room"] and c[2] == ALL for c in st.clones)
        self._room_line(out, a, "here", a["room"], slot, com, as_it_was)
        cov["set_already"] += a["outcome"] in (device.SET_ALREADY_VISIBLE, device.SET_ALREADY_INVISIBLE)
        if a["outcome"] == device.SET_DESC_SET:
            notes["desc"][slot] = inp["inpstr"]
        elif a["outcome"] == device.SET_TOPIC_SET:
            notes["topic"][a["room"]] = inp["inpstr"]
        elif a["outcome"] in (device.SET_INPHR_SET, device.SET_OUTPHR_SET):
            notes["phrase"].add(slot)

    def _access(self, index: int, step: dict, what: str, u: dict, inp: dict, out: dict) -> None:
        """set_room_access, letmein and invite (c:4551-4692): write_user comes first."""
        st, cov, slot, com = self.st, self.res["coverage"], u["slot"], inp["com"]
        a = self.backend.access(slot, com, inp["inpstr"], inp["word_count"])
        self._outcome(index, step, "ACCESS_", a["outcome"])
        if a["texts"]["reply"] is not None:
            out[slot] += b"".join(a["plans"]["reply"]["chunks"][u["colour"]])
        self._room_line(out, a, "here", a["room"], slot, com)
        self._room_line(out, a, "there", a["target_room"], None, com)
        if a["texts"]["notice"] is not None:
            who = a["target_slot"]
            out[who] += b"".join(a["plans"]["notice"]["chunks"][st.users[who]["colour"]])
        if a["outcome"] == device.ACCESS_SET_PUBLIC:
            self._returned_to_public(index, step, a["target_room"])
        done = {"public": (device.ACCESS_SET_PUBLIC,), "private": (device.ACCESS_SET_PRIVATE,), "letmein": (device.ACCESS_ASKED,),
                "invite": (device.ACCESS_INVITED,)}[what]
        cov[{"public": "access", "private": "access"}.get(what, what) + "_refused"] += a["outcome"] not in done

    # -- one step
    def line(self, index: int, step: dict) -> None:
        st, res = self.st, self.res
        u = st.users[st.seats[step["actor"]]]
        data = step["send"].encode("latin-1") + b"\n"
        out = {slot: b"" for slot in st.users}
        self.backend.sync()
        inp = self.backend.input(u["slot"], data, record=True)
        if inp["kind"] == UNKNOWN:
            what = "unknown"
            out[u["slot"]] += b"".join(inp["reply"][u["colour"]])
        elif inp["kind"] == SPEECH:
            what = nuts_path.lib().np_command_name(inp["com"]).decode()
            self._speech(u, inp, out)
        elif inp["kind"] == COMMAND:
            what = nuts_path.lib().np_command_name(inp["com"]).decode()
            if what in ("tell", "pemote"):
                self._tell(u, inp, out)
            elif what == "look":
                self._look(u, out)
            elif what == "who":
                res["coverage"]["who_below_invisible"] += self._below_invisible(u, False)
                out[u["slot"]] += self.backend.who(u["slot"])
                self._shown("desc", [j for j in st.users if j != u["slot"]], out[u["slot"]])
            elif what == "review":
                out[u["slot"]] += self._review(u, inp)
            elif what == "revtell":
                out[u["slot"]] += self._revtell(u)
            elif what in ROOMS_COMMANDS:
                res["coverage"][what] += 1
                out[u["slot"]] += self.backend.rooms(u["slot"], ROOMS_COMMANDS[what])
                if ROOMS_COMMANDS[what]:
                    self._shown("topic", range(len(st.rooms)), out[u["slot"]])
            elif what in GO_COMMANDS:
                self._go(index, step, u, inp, out)
            elif what in CLONE_COMMANDS:
                self._clone(index, step, u, inp, out)
            elif what in SET_COMMANDS:
                self._set(index, step, u, inp, out)
            elif what in ACCESS_COMMANDS:
                self._access(index, step, what, u, inp, out)
            else:
                raise ReplayError(f"step {index}: {step['send']!r} dispatches to .{what}, which the replayer does not answer")
        else:
            raise ReplayError(f"step {index}: {step['send']!r} is a read of kind {inp['kind']}, which the replayer does not answer")
        if u["command_mode"]:                                           # prompt(), nuts333.c:2185-2188
            out[u["slot"]] += nuts_path.transduce(b"~FTCOM> " if u["vis"] else b"~FTCOM+> ", u["colour"])
        res["commands"][what] = res["commands"].get(what, 0) + 1
        res["answered"] += 1
        for actor, slot in st.seats.items():
            got, want = out[slot], step["recv"].get(actor, "").encode("latin-1")
            res["comparisons"] += 1
            if got != want:
                res["mismatches"].append({"step": index, "send": step["send"][:80], "by": step["actor"], "client": actor,
                                          "got": got.decode("latin-1")[:300], "want": want.decode("latin-1")[:300]})
        res["mirror_checks"] += 1
        for m in self.backend.mirror():                                 # what the binding applied, against the state
            res["mismatches"].append({"step": index, "send": step["send"][:80], "by": step["actor"], **m})

    def run(self) -> dict:
        try:
            for i, step in enumerate(self.doc["steps"]):
                if step["op"] == "login":
                    self.st.login(step["actor"], step["name"])
                elif step["op"] == "line":
                    self.line(i, step)
                elif step["op"] != "connect":
                    raise ReplayError(f"step {i}: a {step['op']!r} step")
        finally:
            self.backend.close()
        res = self.res
        res["slots"] = sorted(self.st.users)
        res["calls"] = getattr(self.backend, "calls", {})
        res["uploads"] = getattr(self.backend, "uploads", {})
        return res


def load(seed: int) -> dict:
    return json.loads((GOLDEN / f"replay_{seed}.json").read_text())


def replay(doc: dict, backend_class=ModelBackend, layout: str = COMPACT, **kw) -> dict:
    return Replayer(doc, backend_class, layout, **kw).run()


def coverage_gaps(docs: dict) -> list:
    """What the sessions ``{seed: doc}`` fail to cover (empty: nothing), from a replay of each through the CPU models: the
    generator refuses to write unless this is empty, and tests/test_device_replay.py asserts it of the committed fixtures."""
    missing = []
    total = {k: 0 for k in COVERAGE}
    levels, colours, command_mode, muzzled, fbbm = set(), set(), 0, 0, 0
    for seed, doc in docs.items():
        res = replay(doc)
        if res["mismatches"]:
            missing.append(f"replay_{seed}: the models disagree with the recording: {res['mismatches'][0]}")
        if res["tracked"] or res["answered"] != sum(s["op"] == "line" for s in doc["steps"]):
            missing.append(f"replay_{seed}: {res['answered']} steps answered, {res['tracked']} tracked")
        for k, v in res["coverage"].items():
            total[k] += v
        accounts = doc["accounts"][0]
        if not 4 <= len(accounts) <= 6:
            missing.append(f"replay_{seed}: {len(accounts)} accounts")
        levels |= {a["level"] for a in accounts}
        colours |= {a["colour"] for a in accounts}
        command_mode += any(a["command_mode"] for a in accounts)
        muzzled += any(a["muzzled"] for a in accounts)
        fbbm += any("~FBBM" in a["desc"] for a in accounts)
    missing += [k for k, v in total.items() if not v]
    if levels != {0, 1, 2, 3, 4} or colours != {0, 1} or not command_mode or not muzzled or not fbbm:
        missing.append(f"accounts: levels {sorted(levels)}, colours {sorted(colours)}, command mode {command_mode}, muzzled {muzzled}")
    if sum(bool(d["config"]["ban_swearing"]) for d in docs.values()) * 2 != len(docs):
        missing.append("ban_swearing is not on in half of the sessions")
    return missing
