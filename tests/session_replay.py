"""One replayer for whole recorded sessions: every line step of a session of tests/golden/reference_only/replay_*.json is
answered through the calls of ``device.Roster`` and compared, client by client, with what the reference wrote.

The replayer keeps ONE state for the whole talker -- the users by slot (room, colour, ignall, ignshout, igntell, vis,
muzzled, command_mode, level, name, desc), the clone records in creation order (owner, room, hear), the room table of
``default_rooms()`` -- and a *backend* keeps the review and the revtell rings and answers with one method per Roster
call.  ``ModelBackend`` is built from the CPU models the per-call tests already pin: ``dispatch`` / ``answer_of``
(tests/device_input_child.py), ``model`` of the speech commands behind them, ``private`` and ``TellRings``
(tests/device_tell_child.py), ``look`` (tests/device_look_child.py), ``who`` (tests/device_who_child.py), ``Rings``
(tests/device_review_child.py), ``relays`` / ``relay_text`` (tests/device_relay_child.py) and ``nuts_path.chunks``.
``DeviceBackend`` is one ``Roster(capacity, review_rooms=R, revtell=True, look_rooms=R, clones=C)`` that lives for the
whole session and is updated only with the fields that changed since the last step.

What is taken from the recording, and nothing else: the accounts and the configuration the session was provisioned with,
each step's input line, the bytes to compare against, and whether a ``.go``, a ``.clone`` or a ``.destroy`` succeeded --
read from the actor's recorded bytes, as ``replay_looks`` reads ``Access is ``.

A step is *answered* (every client's bytes are compared, the actor's included) when its line dispatches to speech, to
``tell`` / ``pemote``, ``look``, ``review``, ``revtell`` or ``who``, or to nothing at all (``Unknown command.``).  It is
*tracked* (every client's bytes but the actor's are compared) when it dispatches to ``go``, ``colour``, ``ignall``,
``ignshout``, ``igntell``, ``vis``, ``invis``, ``clone``, ``destroy``, ``chear`` or ``csay``: the broadcasts these make
are composed here from the reference's format strings and delivered through ``relay_many``.  After a ``.go`` that
succeeded, the actor's bytes must begin with what its own clones relayed to it of the move, then the look of its new
room.  A line that dispatches to anything else raises
``ReplayError``; no step is skipped.

Every room line a speech step composes goes through ``input_many(record=True)`` and then, as a broadcast of its own,
through ``relay_many``: the two plans of the same line -- admit bitmap, both variants, chunk sizes -- must be equal.

A clone is a user object in the reference's list: ``look()`` shows it, ``write_room_except`` skips it as a listener and
``get_user`` and ``who()`` pass over it.  The Roster keeps clone records apart from the slots, so the replayer also seats
every clone in a slot of its own behind the last user, in creation order, with the owner's name, the description
``~BR(CLONE)`` and the ``login`` flag: such a slot is listed by ``look_many`` and by nothing else.  A roster therefore
has one slot per possible clone behind the users' slots.

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
from device_look_child import LOOK_MARK, default_rooms  # noqa: E402
from device_look_child import model_chunks as look_chunks  # noqa: E402
from device_look_child import set_rooms  # noqa: E402
from device_relay_child import relay_text, relays, swearing  # noqa: E402
from device_review_child import Rings  # noqa: E402
from device_speak_child import EMOTE, SAY, SEMOTE, SHOUT  # noqa: E402
from device_tell_child import PEMOTE, REVTELL_EMPTY, REVTELL_FOOTER, REVTELL_HEADER, TELL, TellRings, capitalised, get_user, private  # noqa: E402
from device_who_child import model_chunks as who_chunks  # noqa: E402
from nuts333_amd import device, nuts_path  # noqa: E402

GOLDEN = REPO / "tests" / "golden" / "reference_only"
SEEDS = (60, 83, 155, 205, 236, 258, 267, 270)
NOW, DATE = 1000, b"DATE"
ARCH = 3                                                               # gatecrash_level of the generated config
ALL, SWEARS, NOTHING = device.CLONE_HEAR_ALL, device.CLONE_HEAR_SWEARS, device.CLONE_HEAR_NOTHING
HEAR = {b"all": ALL, b"swears": SWEARS, b"nothing": NOTHING}
CLONE_DESC = b"~BR(CLONE)"                                              # nuts333.c:7148
NOSUCHROOM = b"There is no such room.\n"                                # nuts333.h:145
REVIEW_PRIVATE = b"That room is currently private, you cannot review the conversation.\n"   # nuts333.c:5204
REVIEW_HEADER = b"\n~BB~FG*** Review buffer for the %s ***\n\n"         # nuts333.c:5214
REVIEW_FOOTER = b"\n~BB~FG*** End ***\n\n"                              # nuts333.c:5221
REVIEW_EMPTY = b"Review buffer is empty.\n"                             # nuts333.c:5220
CLONE_CREATED, CLONE_DESTROYED = "a clone is created", "the clone is destroyed"     # nuts333.c:7151-7153, 7193
ANSWERED = ("tell", "pemote", "look", "review", "revtell", "who")
TRACKED = ("go", "colour", "ignall", "ignshout", "igntell", "vis", "invis", "clone", "destroy", "chear", "csay")
#: where the users sit, in login order: next to each other, or at the edges of every per-slot lane, ballot word and block
COMPACT, SPREAD = "compact", "spread"
SPREAD_SLOTS = {4: (0, 63, 64, 256), 5: (0, 63, 64, 255, 256), 6: (0, 63, 64, 128, 255, 256)}
COVERAGE = ("say_outside_room_0", "say_relayed", "say_withheld_by_nothing", "swears_clone_swearing", "swears_clone_clean",
            "shout_with_ignshout_listener", "tell_to_igntell", "tell_to_ignall", "tell_by_substring",
            "tell_exact_behind_substring", "line_of_200_bytes", "review_wrapped", "revtell_of_two", "line_past_clone_of_ignall_owner", "look_after_go_below_invisible", "who_below_invisible", "go_refused")


class ReplayError(ValueError):
    """A step the replayer does not know how to answer."""


def words_of(line: bytes) -> list:
    """word[] of wordfind() over ``line``: at most ten words, each cut at 39 bytes."""
    buf = ctypes.create_string_buffer(10 * 41)
    n = nuts_path.lib().np_wordfind(line, buf)
    return [buf.raw[41 * i:41 * (i + 1)].split(b"\0", 1)[0] for i in range(n)]


def both(text):
    return None if text is None else {c: nuts_path.chunks(text, c) for c in (0, 1)}


# ------------------------------------------------------------------ the state
class State:
    def __init__(self, doc: dict, layout: str):
        self.accounts = {a["name"]: a for a in doc["accounts"][0]}
        self.ban = bool(doc["config"].get("ban_swearing", False))
        self.max_clones = int(doc["config"].get("max_clones", 1))
        self.rooms = default_rooms()
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
                            "afk": 0, "afk_mesg": b"", "last_login": NOW, "away": None, "prompt": 0,
                            "in_phrase": enc("in_phrase"), "out_phrase": enc("out_phrase"), "went": False}

    def everyone(self) -> dict:
        """The users and, behind them, the clones as the slots look() lists them from."""
        out = dict(self.users)
        for i, (owner, room, _hear) in enumerate(self.clones):
            slot = self.clone_base + i
            out[slot] = {"slot": slot, "room": room, "login": 1, "colour": 0, "ignall": 0, "ignshout": 0, "igntell": 0, "vis": 1,
                         "muzzled": 0, "level": 0, "command_mode": 0, "name": self.users[owner]["name"], "desc": CLONE_DESC,
                         "afk": 0, "afk_mesg": b"", "last_login": NOW, "away": None}
        return out

    def records(self) -> list:
        return [tuple(c) for c in self.clones]

    def get_room(self, word: bytes):
        return next((i for i, r in enumerate(self.rooms) if r["name"].startswith(word)), None)       # nuts333.c:2388-2389

    def has_room_access(self, u: dict, rm: int) -> bool:                # nuts333.c:2416-2420, nobody is invited
        access = self.rooms[rm]["access"]
        return not (access & 1 and u["level"] < ARCH and not (access & 2 and u["level"] >= 2))

    def find_clone(self, owner: int, rm):
        return next((i for i, c in enumerate(self.clones) if c[0] == owner and c[1] == rm), None)


# ------------------------------------------------------------------ the backends
class ModelBackend:
    """One method per Roster call, from the CPU models of the per-call tests."""

    def __init__(self, st: State):
        self.st = st
        self.rings, self.tells = Rings(len(st.rooms)), TellRings(st.capacity)

    def sync(self) -> None:
        self.all = self.st.everyone()

    def close(self) -> None:
        pass

    def _plan(self, text: bytes, rm, sender, force_listen: int, com: int) -> dict:
        admitted = [j for j, u in sorted(self.all.items())
                    if nuts_path.admits([u["login"], int(u["room"] is not None), int(rm is not None and u["room"] == rm), u["ignall"],
                                         u["ignshout"], int(j == sender)], int(rm is None), force_listen, com)]
        return {"admitted": admitted, "chunks": both(text), "bits": None}

    def input(self, slot: int, data: bytes, record: bool) -> dict:
        d, m = answer_of(self.all[slot], data, self.st.ban)
        if record and m["recorded"]:
            self.rings.record(m["rm"], m["line"])
        return {"kind": d["kind"], "com": d["com"], "word_count": d["word_count"],
                "inpstr": data[d["start"]:d["start"] + d["size"]] if d["size"] >= 0 else b"", "reply": both(m["reply"]),
                "line": m["line"], "plan": None if m["line"] is None else self._plan(m["line"], m["rm"], m["sender"], 0, d["com"])}

    def relay(self, broadcasts, record=None, clone_sender=None) -> list:
        out = []
        ignall = {j: u["ignall"] for j, u in self.all.items()}
        for k, (text, rm, sender, fl, com) in enumerate(broadcasts):
            cs = clone_sender[k] if clone_sender else None
            who = relays(self.st.records(), ignall, rm, cs, text)
            ch = both(relay_text(self.st.rooms[rm]["name"], text)) if who else None
            out.append({"plan": self._plan(text, rm, sender, fl, com), "relays": [(self.st.clones[c][0], ch) for c in who]})
            if record and record[k]:
                self.rings.record(rm, text)
        return out

    def tell(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        m = private(self.all, slot, com, inpstr, word_count)
        if m["line"] is not None:
            self.tells.record(m["target"], m["line"])
        return {"reply": both(m["reply"]), "line": both(m["line"]), "target": m["target"]}

    def look(self, slot: int) -> bytes:
        return b"".join(look_chunks(self.all, self.st.rooms, slot))

    def who(self, slot: int) -> bytes:
        return b"".join(who_chunks(self.all, self.st.rooms, slot, NOW, DATE))

    def review(self, rm: int) -> dict:
        return {"lines": len(self.rings.lines(rm)), **{c: self.rings.chunks(rm, c) for c in (0, 1)}}

    def revtell(self, slot: int) -> dict:
        return {"lines": len(self.tells.lines(slot)), **{c: self.tells.chunks(slot, c) for c in (0, 1)}}


USER_FIELDS = ("room", "login", "colour", "ignall", "ignshout", "igntell", "vis", "muzzled", "level", "command_mode", "name",
               "desc", "last_login")


class DeviceBackend:
    """The same methods over one Roster that lives for the session; ``sync`` uploads what changed, and no more."""

    def __init__(self, st: State):
        self.st = st
        r = len(st.rooms)
        self.roster = device.Roster(st.capacity, review_rooms=r, revtell=True, look_rooms=r, clones=st.clone_seats)
        set_rooms(self.roster, st.rooms)
        self.sent, self.sent_clones = {}, [None] * st.clone_seats
        self.calls = {}

    def close(self) -> None:
        self.roster.close()

    def _count(self, what: str) -> None:
        self.calls[what] = self.calls.get(what, 0) + 1

    def sync(self) -> None:
        now = self.st.everyone()
        for slot in sorted(set(now) | set(self.sent)):
            want = ({f: now[slot][f] for f in USER_FIELDS} if slot in now
                    else {**self.sent[slot], "room": None, "login": 1})             # a clone's slot after its .destroy
            changed = {f: v for f, v in want.items() if slot not in self.sent or self.sent[slot][f] != v}
            if changed:
                self.roster.update(slot, **changed)
                self.sent[slot] = want
        records = self.st.records() + [None] * (self.st.clone_seats - len(self.st.clones))
        for c, rec in enumerate(records):
            if rec != self.sent_clones[c]:
                if rec is None:
                    self.roster.set_clones(c, owner=None)
                else:
                    self.roster.set_clones(c, owner=rec[0], room=rec[1], hear=rec[2])
                self.sent_clones[c] = rec

    def _plan(self, plan: device.Plan, k: int) -> dict:
        return {"admitted": np.flatnonzero(plan.admitted(k)).tolist(), "chunks": {c: plan.chunks(k, c) for c in (0, 1)},
                "bits": plan.admitted_bits[k].tobytes() + b"".join(plan.variant(k, c) for c in (0, 1))}

    def input(self, slot: int, data: bytes, record: bool) -> dict:
        inp = self.roster.input_many([(slot, data)], ban_swearing=self.st.ban, record=record)
        self._count("input_many")
        sp = inp.speech
        return {"kind": int(inp.kind[0]), "com": int(inp.com[0]), "word_count": int(inp.word_count[0]), "inpstr": inp.inpstr(0),
                "reply": {c: sp.reply.chunks(0, c) for c in (0, 1)} if sp.reply_text(0) else None,
                "line": sp.line(0) or None, "plan": self._plan(sp.room, 0) if sp.line(0) else None}

    def relay(self, broadcasts, record=None, clone_sender=None) -> list:
        rl = self.roster.relay_many(broadcasts, record=record, clone_sender=clone_sender)
        self._count("relay_many")
        out = []
        for k in range(len(broadcasts)):
            ch = {c: rl.relay_chunks(k, c) for c in (0, 1)}
            out.append({"plan": self._plan(rl.plan, k), "relays": [(int(o), ch) for o in rl.owners(k)]})
        return out

    def tell(self, slot: int, com: int, inpstr: bytes, word_count: int) -> dict:
        pv = self.roster.tell_many([(slot, com, inpstr, word_count)], record=True)
        self._count("tell_many")
        target = int(pv.target[0])
        return {"reply": {c: pv.reply.chunks(0, c) for c in (0, 1)},
                "line": {c: pv.told.chunks(0, c) for c in (0, 1)} if pv.line(0) else None, "target": None if target < 0 else target}

    def look(self, slot: int) -> bytes:
        self._count("look_many")
        return self.roster.look_many([slot]).output(0)

    def who(self, slot: int) -> bytes:
        self._count("who_many")
        return self.roster.who_many([slot], now=NOW, date=DATE).output(0)

    def review(self, rm: int) -> dict:
        self._count("review_many")
        rv = self.roster.review_many([rm])
        return {"lines": int(rv.line_counts[0]), **{c: rv.chunks(0, c) for c in (0, 1)}}

    def revtell(self, slot: int) -> dict:
        self._count("revtell_many")
        rv = self.roster.revtell_many([slot])
        return {"lines": int(rv.line_counts[0]), **{c: rv.chunks(0, c) for c in (0, 1)}}


# ------------------------------------------------------------------ the replayer
class Replayer:
    def __init__(self, doc: dict, backend_class=ModelBackend, layout: str = COMPACT, everyone_in_room_0: bool = False):
        self.doc = doc
        self.st = State(doc, layout)
        self.backend = backend_class(self.st)
        self.frozen = everyone_in_room_0            # the old replay_reads assumption, kept to show that it now fails
        self.recorded = {}                          # room -> lines recorded into its ring so far
        self.res = {"answered": 0, "tracked": 0, "comparisons": 0, "plan_checks": 0, "plan_disagreements": 0, "mismatches": [],
                    "commands": {}, "coverage": {k: 0 for k in COVERAGE}, "capacity": self.st.capacity, "slots": []}

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
        self.backend.sync()
        parts = self.backend.relay(broadcasts, record=record, clone_sender=clone_sender)
        self._deliver(out, parts)
        cov, st = self.res["coverage"], self.st
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
        here = [c for c in self.st.clones if c[1] == rm and not users[c[0]]["ignall"]]
        if com == SAY:
            cov["say_relayed"] += bool(part["relays"])
            cov["say_withheld_by_nothing"] += any(c[2] == NOTHING for c in here)
        cov["line_past_clone_of_ignall_owner"] += any(c[1] == rm and users[c[0]]["ignall"] and (c[2] == ALL or c[2] == SWEARS and swearing(text))
                                                      for c in self.st.clones)
        if any(c[2] == SWEARS for c in here):
            cov["swears_clone_swearing" if swearing(text) else "swears_clone_clean"] += 1

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

    def _tracked(self, what: str, u: dict, inp: dict, out: dict, mine: str):
        """A command that changes the state: its broadcasts, from the reference's format strings, through relay_many.
        Returns the look a successful .go ends with, else None."""
        st, cov, com = self.st, self.res["coverage"], inp["com"]
        me, slot, words = u["name"], u["slot"], words_of(inp["inpstr"])
        shown = me if u["vis"] else device.INVISNAME
        if what in ("colour", "ignshout", "igntell"):                   # nuts333.c:7472-7479, 7487-7493, 7500-7506
            u[what] ^= 1
        elif what == "ignall":                                          # toggle_ignall, c:4466-4476: the flag flips last
            text = b"%s is now ignoring everyone.\n" % me if not u["ignall"] else b"%s is listening again.\n" % me
            self._broadcast(out, [(text, u["room"], slot, 0, com)])
            u["ignall"] ^= 1
        elif what in ("vis", "invis"):                                  # visibility, c:6438-6454
            if u["vis"] != (what == "vis"):
                text = (b"~FB~OLYou hear a melodic incantation chanted and %s materialises!\n" % me if what == "vis"
                        else b"~FB~OL%s recites a melodic incantation and disappears!\n" % me)
                self._broadcast(out, [(text, u["room"], slot, 0, com)])
                u["vis"] ^= 1
        elif what == "go":                                              # go, c:4384-4404, and move_user, c:4416-4457
            if LOOK_MARK not in mine:
                cov["go_refused"] += bool(words)
                return None
            rm, old = st.get_room(words[0]), u["room"]
            if not u["vis"]:                                            # c:4423-4426
                bs = [(b"A presence enters the room...\n", rm, None, 0, com), (b"A presence leaves the room.\n", old, slot, 0, com)]
            elif rm not in st.rooms[old]["links"]:                      # teleport, c:4428-4433
                bs = [(b"~FT~OL%s appears in an explosion of blue magic!\n" % me, rm, None, 0, com),
                      (b"~FT~OL%s chants a spell and vanishes into a magical blue vortex!\n" % me, old, slot, 0, com)]
            else:                                                       # c:4450-4453
                bs = [(b"%s %s.\n" % (me, u["in_phrase"]), rm, None, 0, com),
                      (b"%s %s to the %s.\n" % (me, u["out_phrase"], st.rooms[rm]["name"]), old, slot, 0, com)]
            self._broadcast(out, bs)
            if not self.frozen:
                u["room"] = rm
            u["went"] = True
            self.backend.sync()
            return self.backend.look(slot)
        elif what == "clone":                                           # create_clone, c:7109-7160
            if CLONE_CREATED in mine:
                rm = st.get_room(words[0]) if words else u["room"]
                st.clones.append([slot, rm, ALL])                       # in the list before the two lines go out
                self._broadcast(out, [(b"~FB~OL%s whispers a haunting spell...\n" % shown, u["room"], slot, 0, com),
                                      (b"~FB~OLA clone of %s appears in a swirling magical mist!\n" % me, rm, slot, 0, com)])
        elif what == "destroy":                                         # destroy_clone, c:7173-7205
            if CLONE_DESTROYED in mine:
                rm = st.get_room(words[0]) if words else u["room"]
                whose = get_user(st.users, words[1]) if len(words) > 1 else slot
                del st.clones[st.find_clone(whose, rm)]
                self._broadcast(out, [(b"~FM~OL%s whispers a sharp spell...\n" % shown, u["room"], slot, 0, com),
                                      (b"~FM~OLThe clone of %s shimmers and vanishes.\n" % st.users[whose]["name"], rm, None, 0, com)])
                if whose != slot:                                       # c:7199-7202
                    out[whose] += nuts_path.transduce(b"~OLSYSTEM: ~FR%s has destroyed your clone in the %s.\n"
                                                      % (me, st.rooms[rm]["name"]), st.users[whose]["colour"])
        elif what == "chear":                                           # clone_hear, c:7328-7356
            if len(words) >= 2 and words[1] in HEAR:
                i = st.find_clone(slot, st.get_room(words[0]))
                if i is not None:
                    st.clones[i][2] = HEAR[words[1]]
        elif what == "csay":                                            # clone_say, c:7300-7316 -> say(clone), c:4085-4088
            if not u["muzzled"] and len(words) >= 2:
                i = st.find_clone(slot, st.get_room(words[0]))
                if i is not None:
                    said = nuts_path.lib().np_remove_first(inp["inpstr"])
                    text = b"Clone of %s %ss: %s\n" % (me, nuts_path.lib().np_say_verb(said), said)
                    self._broadcast(out, [(text, st.clones[i][1], None, 0, com)], record=[True])
        return None

    # -- one step
    def line(self, index: int, step: dict) -> None:
        st, res = self.st, self.res
        u = st.users[st.seats[step["actor"]]]
        data = step["send"].encode("latin-1") + b"\n"
        mine = step["recv"].get(step["actor"], "")
        out = {slot: b"" for slot in st.users}
        self.backend.sync()
        inp = self.backend.input(u["slot"], data, record=True)
        look_after_go, compare_actor = None, True
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
                res["coverage"]["look_after_go_below_invisible"] += u["went"] and self._below_invisible(u, True)
                out[u["slot"]] += self.backend.look(u["slot"])
            elif what == "who":
                res["coverage"]["who_below_invisible"] += self._below_invisible(u, False)
                out[u["slot"]] += self.backend.who(u["slot"])
            elif what == "review":
                out[u["slot"]] += self._review(u, inp)
            elif what == "revtell":
                out[u["slot"]] += self._revtell(u)
            elif what in TRACKED:
                compare_actor = False
                look_after_go = self._tracked(what, u, inp, out, mine)
                if look_after_go is not None:                           # behind what its own clones relayed to it of the move
                    look_after_go = out[u["slot"]] + look_after_go
            else:
                raise ReplayError(f"step {index}: {step['send']!r} dispatches to .{what}, which the replayer does not answer")
        else:
            raise ReplayError(f"step {index}: {step['send']!r} is a read of kind {inp['kind']}, which the replayer does not answer")
        if u["command_mode"]:                                           # prompt(), nuts333.c:2185-2188
            out[u["slot"]] += nuts_path.transduce(b"~FTCOM> " if u["vis"] else b"~FTCOM+> ", u["colour"])
        res["commands"][what] = res["commands"].get(what, 0) + 1
        res["answered" if compare_actor else "tracked"] += 1
        for actor, slot in st.seats.items():
            if slot == u["slot"] and not compare_actor:
                continue
            got, want = out[slot], step["recv"].get(actor, "").encode("latin-1")
            res["comparisons"] += 1
            if got != want:
                res["mismatches"].append({"step": index, "send": step["send"][:80], "by": step["actor"], "client": actor,
                                          "got": got.decode("latin-1")[:300], "want": want.decode("latin-1")[:300]})
        if look_after_go is not None:
            res["comparisons"] += 1
            if not mine.encode("latin-1").startswith(look_after_go):
                res["mismatches"].append({"step": index, "send": step["send"], "client": step["actor"], "what": "the look after .go",
                                          "got": look_after_go.decode("latin-1")[:300], "want": mine[:300]})

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
        res["answered_share"] = res["answered"] / max(1, res["answered"] + res["tracked"])
        res["calls"] = getattr(self.backend, "calls", {})
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
        if res["answered_share"] < 0.6:
            missing.append(f"replay_{seed}: answered share {res['answered_share']:.2f}")
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
