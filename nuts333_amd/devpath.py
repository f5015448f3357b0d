"""What one broadcast's user-space stage costs on the MI355X, done by a kernel that does the work.

    python -m nuts333_amd.devpath [--reps R] [--warmup W] [--pathbench-iterations I] [--per-call K[,K...]]
                                  [--roster K[,K...]] [--plan K[,K...]] [--review Q[,Q...]] [--speak K[,K...]]
                                  [--input K[,K...]] [--tell K[,K...]] [--look K[,K...]] [--relay K[,K...]] [--go K[,K...]]
                                  [--who K[,K...]] [--rooms K[,K...]] [--access K[,K...]] [--clone K[,K...]]
                                  [--set K[,K...]] [--act K[,K...]]                                    -> one JSON line

For N in {10, 100, 1000} listeners, the two texts oracle/pathbench.c times (``say``; ``shout`` carrying ``~OL``/``~RS``)
and colour all-off / all-on / half, one ``nuts333_amd.device.broadcast`` per repetition (listener 0 is the sender, the
rest are admitted: the bench headline's shape).  Per case:

* ``kernels_us``: device events around the fan-out kernels (measure, two rocPRIM scans, emit);
* ``end_to_end_us``: host clock around the listener table + text H2D, the kernels, the results' D2H and a synchronise;
* ``cpu_derived_us``: the CPU user-space time of the same broadcast, DERIVED from ``oracle/_build/pathbench`` run in the
  same call: (N - 1) per-recipient transduces + N predicates + one ``format_line_once``;
* ``bytes_out``: output bytes per broadcast (checked against the CPU restatement once per case).

Median and spread (p10, p90) over the repetitions, after a warm-up.  With no GPU visible the command exits 2; it has
no CPU fall-back.

``--per-call K[,K...]`` adds ``per_call``: the same N x text x colour cases as K broadcasts per call
(``nuts333_amd.device.broadcast_many``), the K texts differing in their line number (000000, 000001, ...).  Per case:
``kernels_us`` and ``end_to_end_us`` per call and per broadcast, ``python_us`` (the host clock around the whole
``broadcast_many`` call: packing the K tables, the library call, copying the results out of pinned memory), and
``cpu_derived_us`` per broadcast with the ratios.  Bytes are checked against the CPU restatement once per case.

``--roster K[,K...]`` adds ``roster``: the same cases through ``nuts333_amd.device.Roster.broadcast_many``, to a roster
of N slots built once per case, untimed (everyone in room 0, slot 0 the sender), so every broadcast is
``(text, 0, 0, 0, COM[text])``.  The same fields as ``per_call``, plus ``h2d_bytes`` uploaded per timed call (no table:
nothing changed) and ``h2d_bytes_first_call`` (with the table).

``--plan K[,K...]`` adds ``plan``: the same cases and rosters through ``nuts333_amd.device.Roster.plan_many``, which
returns the two variants and an admit bitmap per broadcast instead of an arena (one kernel, one download, one
synchronise).  The same fields as ``roster``; ``bytes_out``, ``writes`` and ``recipients`` are counted from the plan
(admitted slots of each colour x that variant's bytes and writes).  ``python_us`` is the host clock around ``plan_many``
alone; the first call's ``expand()`` is checked against the CPU restatement and is not timed.

``--review Q[,Q...]`` adds ``review``: a 1000-slot roster with max(Q) review rings, every ring filled by recording 15
``say`` lines through ``plan_many(record=True)``, then ``Roster.review_many`` of Q rooms per call, for each Q:
``kernels_us``, ``end_to_end_us``, ``python_us``, the copy volume, and the CPU doing the same work, timed in the same
command (``cpu_us``: ``np_transduce`` of the restatement over the same 15 x Q lines, both colours, one ctypes call each;
``cpu_derived_us``: 15 x Q x pathbench's two per-line ``say`` figures, without the calls).  The first review of each Q
is checked against the restatement.  And ``record``: ``plan_many`` of K = 100 to that roster with and without
``record``, alternating in one run.

``--speak K[,K...]`` adds ``speak``: a 1000-slot roster (colour off, on, half) and K ``say`` events per
``Roster.speak_many`` call whose room lines are the K ``say`` texts, timed alternating, in one process, with
``plan_many`` of those K lines composed beforehand: ``kernels_us``, ``end_to_end_us`` and ``python_us`` of both, the
copy volume, what composing adds over ``plan_many``, and the CPU composing the same events (``cpu_us``: ``np_say_verb``,
``np_contains_swearing`` and the two formats of ``say()``, one ctypes call each; ``cpu_derived_us``: 2 x K x pathbench's
``format_line_once_ns``).  The first call of each case is checked against the restatement.

``--input K[,K...]`` adds ``input``: the same rosters and K raw reads per ``Roster.input_many`` call -- the K ``say``
events as their clients send them, ``inpstr`` and a newline -- timed alternating, in one process, with ``speak_many``
of the same events parsed beforehand: the three times and the copy volume of both, what parsing adds over
``speak_many``, and the CPU parsing the same reads with the restatement's functions (``cpu_us``: ``np_terminate`` and
``np_wordfind``, all that ``user_input()`` runs on a plain line; ``cpu_exec_com_us``: those and ``np_remove_first``,
``np_command_lookup`` and ``np_command_level``, the most a read can need; one ctypes call each).  The first call of each
case is checked against ``speak_many`` and the restatement.

``--tell K[,K...]`` adds ``tell``: a 1000-slot roster in which every slot has a name, and K tells of slot 0 to one target
per ``Roster.tell_many`` call, their bodies the K ``say`` bodies, timed alternating, in one process, with ``speak_many``
of K says of the same bodies: the three times and the copy volume of both, and their ratio.  ``get_user`` reads all 1000
slots for every tell.  There is no C restatement of ``get_user`` or ``tell()`` to time beside it:
``cpu_derived_estimate_us`` is 2 x K x pathbench's ``format_line_once_ns``, the two formats alone, an estimate and not
the talker's cost of a tell.  The first call of each case is checked against the reference's two formats.

``--look K[,K...]`` adds ``look``: a 1000-slot roster spread over 5 rooms, 200 users a room, and K looks (slots 0 .. K - 1)
per ``Roster.look_many`` call: the three times and the copy volume, beside ``cpu_us``, the CPU restatement's transducer
(``nuts_path``, through ctypes) over the strings ``look()`` composes for the same lookers.  The strings are composed
beforehand, so ``cpu_us`` leaves the CPU's composing out (``look_cpu_us_covers`` says so).  The first call of each case is
checked against that transducer over those strings.

``--relay K[,K...]`` adds ``relay``: a 1000-slot roster spread over 5 rooms with 64 clone records, of which 0, 1 or 64 stand
in room 0 and hear everything, and K says to room 0 per ``Roster.relay_many`` call, timed alternating, in one process, with
``plan_many`` of the same K broadcasts: the three times and the copy volume of both, and their ratio.  ``cpu_us`` is the
CPU doing ``clone_relay``'s work through ``nuts_path``: per relaying clone the swear scan and the transducer over the
prefixed text (``relay_cpu_us_covers`` says what that leaves out); with no relaying clone there is none.  The first call
of each case is checked against that transducer over the prefixed text.

``--who K[,K...]`` adds ``who``: the 1000-slot roster of ``--look``, every slot a listed user logged in at its own second,
and K whos (slots 0 .. K - 1) per ``Roster.who_many`` call: the three times and the copy volume, beside ``cpu_us``, the
CPU composing ``who()``'s 1003 strings for each looker -- in Python, ``colour_com_count`` included -- and the CPU
restatement's transducer over them (``who_cpu_us_covers`` says what that is worth).  The first call of each case is
checked against that transducer over those strings.

``--rooms K[,K...]`` adds ``rooms``: a 1000-slot roster over the 6 default rooms and one over 1,024 rooms, and K lookers of
one kind (``.rmst``, then ``.rmsn``) per ``Roster.rooms_many`` call: the three times and the copy volume, beside ``cpu_us``,
the CPU composing ``rooms()``'s strings for each looker in Python and the CPU restatement's transducer over them
(``rooms_cpu_us_covers`` says what that is worth).  The first call of each case is checked against that transducer over
those strings.

``--go K[,K...]`` adds ``go``: a 1000-slot roster of WIZ users over the six default rooms, and K walks (slots 0 .. K - 1, each
to a room that adjoins its own both ways) per ``Roster.go_many`` call, there in one call and back in the next, so that the
state is periodic: the three times and the copy volume of both device visits added up, beside ``parts`` -- ``plan_many`` of
the same composed lines, then ``look_many`` of the same movers, which is what a ``go_many`` call is made of -- and ``cpu_us``,
the CPU composing the strings in Python and transducing them.  Six rooms hold at most three disjoint walks, so of K = 8 or
64 events most are deferred: ``moved`` and ``deferred`` say how many.  The first call of each case is checked against the
reference's formats and the CPU's transducer over ``look()``'s strings.

``--access K[,K...]`` adds ``access``: a 1000-slot roster of USERs over the six default rooms, and K ``.private`` events per
``Roster.access_many`` call, each by an actor in its own room (``access_actors``: the first three stand in the three rooms
that can be set), then K ``.public`` events by the same actors in the next call, so that the state is periodic and every
call sets an access: the three times and the copy volume of the ``.private`` call (``public`` has the other's), beside
``plan`` -- ``plan_many`` of the lines the ``.private`` call composes, composed beforehand, in the same rounds -- and
``cpu_us``, the CPU modelling the call in Python and transducing the lines through ctypes.  Three rooms can be set, three
are fixed, so of K = 8 or 64 events most are refused or deferred: ``set``, ``refused`` and ``deferred`` say how many.  Both
calls of each case are checked first against the model, the reference's formats and the CPU's transducer.

``--clone K[,K...]`` adds ``clone``: a 1000-slot roster of ARCHs over the six default rooms with a clone record for each of
the first K users, and K ``.csay`` events per ``Roster.clone_many`` call, each by another owner through its clone: the three
times and the copy volume of that call, beside ``speak`` -- ``speak_many`` of the same bodies as says by the same users, in
the same rounds -- and ``cpu_us``, the CPU composing the lines in Python and transducing them through ctypes;
``csay_over_speak`` is the ratio of the medians, ``csay_over_speak_p10_p90`` the loosest the rounds allow.  Then, in rounds of
their own, ``clone`` -- K ``.clone`` events by K users who own none, each in its own room -- and ``destroy`` -- K ``.destroy``
events by the same users, which returns the records to their start.  Six rooms take six clones a call, so of K = 8 or 64
events most are deferred: ``created`` and ``deferred`` say how many.  Every call is checked first against the reference's
formats, the CPU's transducer and the rule of the call.

``--set K[,K...]`` adds ``set``: a 1000-slot roster of USERs over the six default rooms, and per ``Roster.set_many`` call K
``.ignall`` events by K actors (``ignall``) and K ``.desc <text>`` events by the same actors (``desc``): the three times and
the copy volume of each call, each beside ``speak`` -- ``speak_many`` of the same bodies as says by the same users, in the
same rounds -- and ``cpu_us``, the CPU composing the lines in Python and transducing them through ctypes;
``ignall_over_speak`` and ``desc_over_speak`` are the ratios of the medians, ``..._p10_p90`` the loosest the rounds allow.
An ``.ignall`` changes who hears its room, so the first actor of a room is answered and the later ones of that room wait:
of K = 8 or 64 events six toggle, ``toggled`` and ``deferred`` say how many.  What a call changes travels with the next call
that reads it: the ``.desc`` call uploads the descriptions its last call changed, 32 bytes a slot, with the speaker table
that lies behind them, 16, and in the ``.ignall`` rounds it is ``speak_many`` that uploads the table the ``.ignall`` call
changed, 5 bytes a slot (``h2d_bytes`` shows both).
Both calls are checked first against the reference's formats, the CPU's transducer and the rule of the call.

``--act K[,K...]`` adds ``act``: a 1000-slot roster over the six default rooms whose first half are WIZes and whose second
half are USERs, and per ``Roster.act_many`` call K ``.wake`` events by K actors, each of another user (``wake``), and K
``.move <user> <room>`` events by K WIZ actors, each of another USER into the room behind its own (``move``), with the moves
back in the next call (``back``), so that the state is periodic: the three times and the copy volume of each call -- of
both device visits of a call that moves, added up --, each beside ``parts`` -- ``plan_many`` of the lines the call
composes, composed beforehand, then, for the moves, ``look_many`` of the same users, in the same rounds -- and ``cpu_us``,
the CPU modelling the call in Python and transducing the lines, and the looks, through ctypes.  A wake changes nothing, so
every one is answered; a move touches a slot and two rooms, and its actor's room counts too, so six rooms take two moves
a call: ``moved``, ``already`` and ``deferred`` say how many.  Every call is checked first against the model, the
reference's formats and the CPU's transducer.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path
from typing import NamedTuple

import numpy as np

from nuts333_amd import device, nuts_path

REPO = Path(__file__).resolve().parent.parent
PATHBENCH = REPO / "oracle" / "_build" / "pathbench"

#: the texts oracle/pathbench.c times (its snprintf formats, line number 123)
TEXTS = {
    "say": b"Uaaa says: synthetic broadcast line 000123 from the nuts333 bench\n",
    "shout": b"~OLUaaa shouts:~RS synthetic broadcast line 000123 from the nuts333 bench\n",
}
COM = {"say": device.COM_SAY, "shout": device.COM_SHOUT}
SIZES = (10, 100, 1000)
COLOURS = ("off", "on", "half")


def listeners(n: int, colour: str) -> np.ndarray:
    """n listeners in the sender's room; listener 0 is the sender; colour off / on / every other one."""
    t = np.zeros((n, len(device.LISTENER_FIELDS)), dtype=np.uint8)
    t[:, device.LISTENER_FIELDS.index("has_room")] = 1
    t[:, device.LISTENER_FIELDS.index("same_room")] = 1
    t[0, device.LISTENER_FIELDS.index("is_sender")] = 1
    c = device.LISTENER_FIELDS.index("colour")
    t[:, c] = {"off": 0, "on": 1}.get(colour, 0)
    if colour == "half":
        t[1::2, c] = 1
    return t


def colours(n: int, colour: str) -> np.ndarray:
    """The colour flag of each of listeners(n, colour)."""
    return listeners(n, colour)[:, device.LISTENER_FIELDS.index("colour")]


def _stats(xs: list[float]) -> dict:
    q = np.percentile(xs, [10, 90])
    return {"median": round(statistics.median(xs), 2), "p10": round(float(q[0]), 2), "p90": round(float(q[1]), 2)}


FIELDS = ("kernels_us", "end_to_end_us", "python_us")


class _Step(NamedTuple):
    """What ``_timed`` found for one step."""
    times: dict     # the _stats of kernels_us and end_to_end_us, where the results had a timing, and of python_us
    copied: dict    # the h2d_bytes and d2h_bytes of every kept call, where the timings had them

    @property
    def host_us(self) -> dict:
        """The host clock round the step: ``python_us`` of a device call, what a section prints as ``cpu_us`` of CPU work."""
        return self.times["python_us"]

    @property
    def fields(self) -> dict:
        return {**self.times, **self.copied}


def _timed(label: str, steps: dict, reps: int, warmup: int) -> dict:
    """The timed loop of every section.  A round calls every one of ``steps`` (name -> callable of no arguments) once, in
    order; of ``warmup + reps`` rounds the last ``reps`` are kept.  Kept per step: the host clock round the call and nothing
    else (``python_us``), the ``kernels_us`` and ``end_to_end_us`` of the result's ``timing`` where it has one, and that
    timing's ``(h2d_bytes, d2h_bytes)`` where it has them.  A step whose kept calls did not all copy the same volume ends
    the command.  Returns a ``_Step`` per step."""
    kept = {name: {"kernels_us": [], "end_to_end_us": [], "python_us": [], "copies": set()} for name in steps}
    for i in range(warmup + reps):
        for name, step in steps.items():
            t0 = time.perf_counter()
            r = step()
            us = (time.perf_counter() - t0) * 1e6
            timing = getattr(r, "timing", None)
            if i >= warmup:
                kept[name]["python_us"].append(us)
                if timing:
                    kept[name]["kernels_us"].append(timing["kernels_us"])
                    kept[name]["end_to_end_us"].append(timing["end_to_end_us"])
                    if "h2d_bytes" in timing:
                        kept[name]["copies"].add((timing["h2d_bytes"], timing["d2h_bytes"]))
    out = {}
    for name, lists in kept.items():
        copies = lists.pop("copies")
        if len(copies) > 1:
            raise SystemExit(f"devpath: {label}: timed {name} calls copied {sorted(copies)} bytes")
        out[name] = _Step({f: _stats(xs) for f, xs in lists.items() if xs},
                          dict(zip(("h2d_bytes", "d2h_bytes"), next(iter(copies), ()))))
    return out


def _adds(a: _Step, b: _Step, per: int = 1, digits: int = 2) -> dict:
    """What step ``a`` takes over step ``b``, median from median, per field."""
    return {f: round((a.times[f]["median"] - b.times[f]["median"]) / per, digits) for f in FIELDS}


def _listing_fields(label: str, name: str, call, cpu, first, k: int, reps: int, warmup: int) -> dict:
    """What the cases of the three listing sections (look, who, rooms) share: the bytes and writes of the ``first`` result's K
    listings, then ``call()`` timed as step ``name`` in rounds with ``cpu()``, the CPU doing the same work."""
    timed = _timed(label, {name: call, "cpu": cpu}, reps, warmup)
    dev, cpu_us = timed[name], timed["cpu"].host_us
    return {"bytes_out": sum(len(first.output(i)) for i in range(k)), "writes": sum(len(first.chunks(i)) for i in range(k)),
            **dev.times, "cpu_us": cpu_us, **dev.copied,
            # three significant digits: the ratio is far below 1 when many lines go through ctypes
            "end_to_end_over_cpu": float(f"{dev.times['end_to_end_us']['median'] / cpu_us['median']:.3g}")}


def pathbench(iterations: int) -> dict:
    p = subprocess.run([str(PATHBENCH), str(iterations)], stdout=subprocess.PIPE, check=True, timeout=600)
    return json.loads(p.stdout.decode())


def cpu_derived_us(pb: dict, text: str, colour: str, n: int) -> float:
    """(N - 1) transduces + N predicates + one format_line_once, from pathbench's per-recipient figures."""
    on, off = pb[f"transduce_{text}_colour_on_ns"], pb[f"transduce_{text}_colour_off_ns"]
    per = {"off": off, "on": on, "half": (on + off) / 2}[colour]
    return ((n - 1) * per + n * pb["fanout_predicate_ns"] + pb["format_line_once_ns"]) / 1e3


def per_call_counts(s: str) -> list[int]:
    """``--per-call``: broadcasts per call, comma-separated positive integers."""
    try:
        ks = [int(x) for x in s.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected positive integers separated by commas, got {s!r}") from None
    if any(k < 1 for k in ks):
        raise argparse.ArgumentTypeError(f"broadcasts per call must be >= 1, got {s!r}")
    return ks


def line_texts(text: str, k: int) -> list[bytes]:
    """K distinct texts of one length: TEXTS[text] with line numbers 000000 .. k - 1."""
    if k > 1_000_000:
        raise ValueError("six-digit line numbers: at most 1,000,000 distinct texts")
    return [TEXTS[text].replace(b"000123", b"%06d" % i) for i in range(k)]


def per_call_case(n: int, text: str, colour: str, k: int, reps: int, warmup: int, pb: dict) -> dict:
    """K broadcasts of ``text`` (distinct line numbers) to listeners(n, colour) per broadcast_many call."""
    table = listeners(n, colour)
    calls = [(t, table, 0, 0, COM[text]) for t in line_texts(text, k)]
    return _timed_calls("per call", n, text, colour, k, lambda: device.broadcast_many(calls), reps, warmup, pb)[0]


def roster_case(n: int, text: str, colour: str, k: int, reps: int, warmup: int, pb: dict, plan: bool = False) -> dict:
    """K broadcasts of ``text`` per Roster.broadcast_many call (``plan``: per Roster.plan_many call), to a roster
    built once, untimed, in the listeners(n, colour) shape: every slot in room 0, slot 0 the sender."""
    with device.Roster(n) as roster:
        roster.update(range(n), room=0, colour=colours(n, colour))
        calls = [(t, 0, 0, 0, COM[text]) for t in line_texts(text, k)]
        run = (lambda: roster.plan_many(calls)) if plan else (lambda: roster.broadcast_many(calls))
        case, first, copied = _timed_calls("plan" if plan else "roster", n, text, colour, k, run, reps, warmup, pb,
                                           _plan_totals if plan else _fanout_totals)
    h2d = copied["h2d_bytes"]
    return {**case, "h2d_bytes": h2d, "h2d_bytes_per_broadcast": round(h2d / k, 1),
            "h2d_bytes_first_call": first["h2d_bytes"], "d2h_bytes": first["d2h_bytes"]}


def plan_case(n: int, text: str, colour: str, k: int, reps: int, warmup: int, pb: dict) -> dict:
    """roster_case through Roster.plan_many."""
    return roster_case(n, text, colour, k, reps, warmup, pb, plan=True)


def _fanout_totals(r: device.Fanout):
    """A Fanout's arena, admitted items, bytes and writes."""
    return r.arena.tobytes(), int(r.admitted.sum()), int(r.out_offsets[-1]), int(r.write_offsets[-1])


def _plan_totals(p: device.Plan):
    """The same of a Plan: the arena from expand(), for the check; the counts from the plan itself, admitted slots of
    each colour x that variant's bytes and writes."""
    count = np.array([[len(p.recipients(k, c)) for c in (0, 1)] for k in range(len(p.admitted_bits))], dtype=np.int64)
    return (p.expand().arena.tobytes(), int(count.sum()), int((count * p.variant_sizes).sum()),
            int((count * p.write_counts).sum()))


def _timed_calls(label: str, n: int, text: str, colour: str, k: int, run, reps: int, warmup: int, pb: dict,
                 totals=_fanout_totals):
    """One case: ``run()`` makes K broadcasts of ``text`` to listeners(n, colour); its first result is checked against
    the CPU restatement (``totals``: its arena, admitted items, bytes and writes), then it is warmed up and timed.
    Returns the case, the first call's timing and the copy volume of the timed calls."""
    texts = line_texts(text, k)
    first = run()
    arena, admitted, bytes_out, writes = totals(first)
    colour_of = colours(n, colour)[1:].tolist()
    want = b"".join(b"".join(v[c] for c in colour_of)
                    for v in ({0: nuts_path.transduce(t, 0), 1: nuts_path.transduce(t, 1)} for t in texts))
    if arena != want or admitted != k * (n - 1) or bytes_out != len(want):
        raise SystemExit(f"devpath: {label} {k}, {n}/{text}/{colour}: device produced {bytes_out} "
                         f"bytes, the CPU restatement {len(want)}")
    timed = _timed(f"{label} {k}, {n}/{text}/{colour}", {label: run}, reps, warmup)[label]
    cpu = cpu_derived_us(pb, text, colour, n)
    case = {"n": n, "text": text, "colour": colour, "k": k, "recipients": k * (n - 1),
            "bytes_out": bytes_out, "writes": writes, **timed.times,
            **{f"{f}_per_broadcast": {q: round(v / k, 3) for q, v in s.items()} for f, s in timed.times.items()},
            "cpu_derived_us": round(cpu, 3),
            "end_to_end_over_cpu": round(timed.times["end_to_end_us"]["median"] / k / cpu, 2),
            "python_over_cpu": round(timed.host_us["median"] / k / cpu, 2)}
    return case, first.timing, timed.copied


def review_cases(qs: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``review`` section: review_many of Q rooms for each Q, and plan_many of K = 100 with and without record."""
    rings = max(qs)
    n, k = 1000, 100
    lib = nuts_path.lib()
    with device.Roster(n, review_rooms=rings) as roster:
        roster.update(range(n), room=0)
        lines = line_texts("say", device.REVIEW_LINES * rings)
        roster.plan_many([(t, i // device.REVIEW_LINES, 0, 0, COM["say"]) for i, t in enumerate(lines)], record=True)
        cases = []
        for q in qs:
            rooms = list(range(q))
            mine = lines[:device.REVIEW_LINES * q]
            first = roster.review_many(rooms)
            for room in rooms:
                own = mine[device.REVIEW_LINES * room:device.REVIEW_LINES * (room + 1)]
                for c in (0, 1):
                    if first.variant(room, c) != b"".join(nuts_path.transduce(t, c) for t in own):
                        raise SystemExit(f"devpath: review {q}: room {room}, colour {c} differs from the CPU restatement")
            out = ctypes.create_string_buffer(device.MAX_LINE_BYTES)

            def cpu_work():
                for t in mine:
                    lib.np_transduce(t, 0, out, len(out))
                    lib.np_transduce(t, 1, out, len(out))
            timed = _timed(f"review {q}", {"review": lambda: roster.review_many(rooms)}, reps, warmup)["review"]
            cpu = _timed(f"review {q}", {"cpu": cpu_work}, reps, warmup)["cpu"].host_us
            es = timed.times["end_to_end_us"]
            derived = len(mine) * (pb["transduce_say_colour_off_ns"] + pb["transduce_say_colour_on_ns"]) / 1e3
            cases.append({"q": q, "lines": len(mine), "bytes_out": int(first.variant_sizes.sum()),
                          "writes": int(first.write_counts.sum()), "sequential": int(first.sequential.sum()),
                          **timed.fields, "cpu_us": cpu, "cpu_derived_us": round(derived, 3),
                          "end_to_end_over_cpu": round(es["median"] / cpu["median"], 2),
                          "end_to_end_over_cpu_derived": round(es["median"] / derived, 2)})
        calls = [(t, 0, 0, 0, COM["say"]) for t in line_texts("say", k)]
        timed = _timed("record", {"without_record": lambda: roster.plan_many(calls),
                                  "with_record": lambda: roster.plan_many(calls, record=True)}, reps, warmup)
        record = {"n": n, "k": k, "text": "say", "room": 0, **{name: step.times for name, step in timed.items()},
                  "record_adds_us": _adds(timed["with_record"], timed["without_record"])}
    return {"review_kernels": ["nuts_roster_review"], "record_kernels": ["nuts_roster_plan", "nuts_roster_record"],
            "review_end_to_end_covers": "one H2D of the Q rooms, one kernel, one D2H of the rings' lines, both variants "
                                        "and their chunk sizes at their bound size (about 40 KB per room), one "
                                        "synchronise (python_us adds checking the rooms, the copies out of pinned "
                                        "memory and building the Review)",
            "review_rings": rings, "review": cases, "record": record}


def speak_events(k: int) -> list[tuple]:
    """K ``say`` events of slot 0 whose room lines are ``line_texts("say", k)``: the speaker is named as TEXTS["say"]
    names it, and ``inpstr`` is what follows "Uaaa says: " without the newline."""
    head = b"Uaaa says: "
    return [(0, device.COM_SAY, t[len(head):-1], 8) for t in line_texts("say", k)]


def speak_cpu_us(events, reps: int, warmup: int) -> dict:
    """The CPU composing the same K says, timed here: per event np_say_verb, np_contains_swearing and the two formats of
    say() (nuts333.c:4094,4097) by the C library's snprintf, one ctypes call each."""
    lib, libc = nuts_path.lib(), ctypes.CDLL(None)
    out, size = ctypes.create_string_buffer(device.TEXT_SIZE), ctypes.c_size_t(device.TEXT_SIZE)

    def compose():
        for _, _, inpstr, _ in events:
            verb = lib.np_say_verb(inpstr)
            lib.np_contains_swearing(inpstr)
            libc.snprintf(out, size, b"You %s: %s\n", ctypes.c_char_p(verb), ctypes.c_char_p(inpstr))
            libc.snprintf(out, size, b"%s %ss: %s\n", ctypes.c_char_p(b"Uaaa"), ctypes.c_char_p(verb),
                          ctypes.c_char_p(inpstr))
    return _timed("speak", {"cpu": compose}, reps, warmup)["cpu"].host_us


def speak_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``speak`` section: speak_many of K says to a 1000-slot roster, alternating with plan_many of the same K
    lines composed beforehand, for each colour case and each K."""
    n = 1000
    cases = []
    for colour in COLOURS:
        with device.Roster(n) as roster:
            roster.update(range(n), room=0, colour=colours(n, colour))
            roster.update(0, name=b"Uaaa")
            for k in ks:
                events, lines = speak_events(k), line_texts("say", k)
                calls = [(t, 0, 0, 0, COM["say"]) for t in lines]
                first, plan = roster.speak_many(events, ban_swearing=True), roster.plan_many(calls)
                for i, t in enumerate(lines):
                    ok = (first.outcome[i] == device.SPOKEN and first.line(i) == t
                          and first.reply_text(i) == b"You say: " + events[i][2] + b"\n"
                          and np.array_equal(first.room.admitted_bits[i], plan.admitted_bits[i])
                          and all(first.room.variant(i, c) == nuts_path.transduce(t, c) == plan.variant(i, c)
                                  and first.reply.variant(i, c) == nuts_path.transduce(first.reply_text(i), c)
                                  for c in (0, 1)))
                    if not ok:
                        raise SystemExit(f"devpath: speak {k}, {colour}: event {i} differs from the CPU restatement")
                sp, pl = _timed(f"speak {k}, {colour}", {"speak": lambda: roster.speak_many(events, ban_swearing=True),
                                                         "plan": lambda: roster.plan_many(calls)}, reps, warmup).values()
                cpu = speak_cpu_us(events, reps, warmup)
                derived = 2 * k * pb["format_line_once_ns"] / 1e3
                cases.append({"n": n, "k": k, "text": "say", "colour": colour, "ban_swearing": True,
                              "recipients": k * (n - 1), **sp.fields, "plan_many_of_the_composed_lines": pl.fields,
                              "composing_adds_us": _adds(sp, pl), "composing_adds_us_per_event": _adds(sp, pl, k, 3),
                              "cpu_us": cpu, "cpu_derived_us": round(derived, 3),
                              "composing_adds_end_to_end_over_cpu":
                                  round((sp.times["end_to_end_us"]["median"] - pl.times["end_to_end_us"]["median"])
                                        / cpu["median"], 2)})
    return {"speak_kernels": ["nuts_roster_speak", "nuts_roster_speak_plan"],
            "speak_end_to_end_covers": "packing the K events into pinned memory, one H2D (the table and the speaker "
                                       "state only in a call after an update of theirs), two kernels, one D2H of the "
                                       "outcomes, the composed texts, both plans' variants and chunk sizes and the admit "
                                       "bitmap at their bound size, one synchronise (python_us adds checking the K "
                                       "events and their speakers, the copies out of pinned memory and building the "
                                       "Speech)",
            "speak_cpu_us_covers": "np_say_verb + np_contains_swearing + the two snprintf formats of say() per event, "
                                   "one ctypes call each; cpu_derived_us is 2 x K x pathbench's format_line_once_ns, "
                                   "without the calls and without the verb and the swear scan",
            "speak": cases}


def input_reads(k: int) -> list[tuple]:
    """The K reads whose parse is ``speak_events(k)``: slot 0's plain lines, each ``inpstr`` and a newline."""
    return [(slot, inpstr + b"\n") for slot, _, inpstr, _ in speak_events(k)]


def input_cpu_us(reads, reps: int, warmup: int, exec_com: bool) -> dict:
    """The CPU parsing the same K reads, timed here: np_terminate on a copy of the read and np_wordfind, as user_input()
    does for a plain line; with ``exec_com`` also np_remove_first, np_command_lookup and np_command_level on the first
    word, as exec_com() would; one ctypes call each."""
    lib = nuts_path.lib()
    words = ctypes.create_string_buffer(10 * 41)
    bufs = [ctypes.create_string_buffer(data, len(data) + 1) for _, data in reads]
    runs = []
    for _ in range(warmup + reps):
        for buf, (_, data) in zip(bufs, reads):                # np_terminate cuts in place: a fresh copy per run
            ctypes.memmove(buf, data, len(data))
        t0 = time.perf_counter()
        for buf in bufs:
            lib.np_terminate(buf)
            lib.np_wordfind(buf, words)
            if exec_com:
                lib.np_remove_first(buf)
                lib.np_command_level(lib.np_command_lookup(words))
        runs.append((time.perf_counter() - t0) * 1e6)
    return _stats(runs[warmup:])


def input_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``input`` section: input_many of K raw reads to a 1000-slot roster, alternating with speak_many of the same
    events parsed beforehand, for each colour case and each K."""
    n = 1000
    cases = []
    for colour in COLOURS:
        with device.Roster(n) as roster:
            roster.update(range(n), room=0, colour=colours(n, colour))
            roster.update(0, name=b"Uaaa", level=1)
            for k in ks:
                reads, events, lines = input_reads(k), speak_events(k), line_texts("say", k)
                first, spoken = roster.input_many(reads, ban_swearing=True), roster.speak_many(events, ban_swearing=True)
                for i, t in enumerate(lines):
                    a, b = first.speech, spoken
                    ok = (first.kind[i] == device.SPEECH and first.com[i] == device.COM_SAY
                          and first.inpstr(i) == events[i][2] and first.word_count[i] == events[i][3]
                          and a.outcome[i] == b.outcome[i] == device.SPOKEN and a.line(i) == b.line(i) == t
                          and a.reply_text(i) == b.reply_text(i)
                          and np.array_equal(a.room.admitted_bits[i], b.room.admitted_bits[i])
                          and all(a.room.variant(i, c) == nuts_path.transduce(t, c) == b.room.variant(i, c)
                                  and a.reply.variant(i, c) == b.reply.variant(i, c) for c in (0, 1)))
                    if not ok:
                        raise SystemExit(f"devpath: input {k}, {colour}: read {i} differs from speak_many of its event")
                ip, sp = _timed(f"input {k}, {colour}", {"input": lambda: roster.input_many(reads, ban_swearing=True),
                                                         "speak": lambda: roster.speak_many(events, ban_swearing=True)},
                                reps, warmup).values()
                cpu = input_cpu_us(reads, reps, warmup, False)
                cases.append({"n": n, "k": k, "text": "say", "colour": colour, "ban_swearing": True,
                              "recipients": k * (n - 1), **ip.fields, "speak_many_of_the_parsed_events": sp.fields,
                              "parsing_adds_us": _adds(ip, sp), "parsing_adds_us_per_read": _adds(ip, sp, k, 3),
                              "cpu_us": cpu, "cpu_exec_com_us": input_cpu_us(reads, reps, warmup, True),
                              "parsing_adds_end_to_end_over_cpu":
                                  round((ip.times["end_to_end_us"]["median"] - sp.times["end_to_end_us"]["median"])
                                        / cpu["median"], 2)})
    return {"input_kernels": ["nuts_roster_parse", "nuts_roster_speak", "nuts_roster_speak_plan"],
            "input_end_to_end_covers": "packing the K reads into pinned memory, one H2D (the table and the speaker state "
                                       "only in a call after an update of theirs), three kernels, one D2H of what the "
                                       "parse found and of all that speak_many downloads, at the bound size, one "
                                       "synchronise (python_us adds checking the K reads and their speakers, the copies "
                                       "out of pinned memory and building the Input)",
            "input_cpu_us_covers": "np_terminate + np_wordfind per read, one ctypes call each: what user_input() runs "
                                   "on a plain line; cpu_exec_com_us adds np_remove_first, np_command_lookup and "
                                   "np_command_level, the most a read can need",
            "input": cases}


TELL_TARGET = (500, b"Zebedee")


def tell_events(k: int) -> list[tuple]:
    """K tells of slot 0 to TELL_TARGET whose bodies are the K says of ``speak_events(k)``: ``inpstr`` is what
    ``.tell zebedee <body>`` hands to tell()."""
    return [(0, device.COM_TELL, TELL_TARGET[1].lower() + b" " + inpstr, 9) for _, _, inpstr, _ in speak_events(k)]


def tell_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``tell`` section: tell_many of K tells to one target in a 1000-slot roster in which every slot has a name,
    alternating with speak_many of K says of the same bodies, for each colour case and each K."""
    n = 1000
    cases = []
    for colour in COLOURS:
        with device.Roster(n) as roster:
            roster.update(range(n), room=0, colour=colours(n, colour),
                          name=[b"User%d" % j for j in range(n)])
            roster.update(0, name=b"Uaaa")
            roster.update(TELL_TARGET[0], name=TELL_TARGET[1])
            for k in ks:
                tells, says = tell_events(k), speak_events(k)
                first = roster.tell_many(tells)
                for i, (_, _, body, _) in enumerate(says):
                    verb = b"ask" if body.endswith(b"?") else b"tell"
                    line = b"~OLUaaa %ss you:~RS %s\n" % (verb, body)
                    reply = b"~OLYou %s %s:~RS %s\n" % (verb, TELL_TARGET[1], body)
                    ok = (first.outcome[i] == device.TOLD and first.target[i] == TELL_TARGET[0] and first.line(i) == line
                          and first.reply_text(i) == reply
                          and first.told.admitted(i).nonzero()[0].tolist() == [TELL_TARGET[0]]
                          and all(first.told.variant(i, c) == nuts_path.transduce(line, c)
                                  and first.reply.variant(i, c) == nuts_path.transduce(reply, c) for c in (0, 1)))
                    if not ok:
                        raise SystemExit(f"devpath: tell {k}, {colour}: event {i} differs from the reference's formats")
                tl, sp = _timed(f"tell {k}, {colour}", {"tell": lambda: roster.tell_many(tells),
                                                        "speak": lambda: roster.speak_many(says, ban_swearing=True)},
                                reps, warmup).values()
                cases.append({"n": n, "k": k, "colour": colour, "target": TELL_TARGET[0], "recipients": k, **tl.fields,
                              "speak_many_of_the_same_bodies": sp.fields,
                              "tell_over_speak": {f: round(tl.times[f]["median"] / sp.times[f]["median"], 2) for f in FIELDS},
                              "cpu_derived_estimate_us": round(2 * k * pb["format_line_once_ns"] / 1e3, 3)})
    return {"tell_kernels": ["nuts_roster_tell", "nuts_roster_speak_plan"],
            "tell_end_to_end_covers": "packing the K events into pinned memory, one H2D (the table, the speaker state and "
                                      "the AFK messages only in a call after an update of theirs), two kernels -- "
                                      "get_user over all 1000 slots per event, the texts, their variants --, one D2H of "
                                      "the outcomes, the targets, the composed texts and both plans' variants and chunk "
                                      "sizes at their bound size, one synchronise (python_us adds checking the K events "
                                      "and their speakers, the copies out of pinned memory and building the Private)",
            "tell_cpu_derived_estimate_us_covers": "an estimate, not a measurement: 2 x K x pathbench's "
                                                   "format_line_once_ns, the two formats of tell() alone, without "
                                                   "get_user's two passes over the user list, which no C restatement "
                                                   "here times",
            "tell": cases}


LOOK_ROOMS = (b"drive", b"hallway", b"wizroom", b"corridor", b"lounge")


def look_strings(n: int, slot: int) -> list[bytes]:
    """What look() hands to write_user for ``slot`` of the roster ``look_cases`` builds: n slots spread over the five
    rooms, slot j in room j % 5, every user visible, of one level and not AFK, each room linked to the next."""
    rm = slot % len(LOOK_ROOMS)
    nxt = (rm + 1) % len(LOOK_ROOMS)
    lines = [b"      User%d is user %d~RS  \n" % (j, j) for j in range(rm, n, len(LOOK_ROOMS)) if j != slot]
    return ([b"\n~FTRoom: ~FG%s\n\n" % LOOK_ROOMS[rm], b"The %s.\nA second line of description.\n" % LOOK_ROOMS[rm],
             b"\n~FTExits are:  ~FG%s\n\n" % LOOK_ROOMS[nxt]]
            + ([b"~FTYou can see:\n"] + lines if lines else [b"~FTYou are all alone here.\n"])
            + [b"\n", b"Access is set to ~FGPUBLIC~RS and there are ~OL~FM%d~RS messages on the board.\n" % rm,
               b"Current topic: the topic of room %d\n" % rm])


def look_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``look`` section: look_many of K lookers (slots 0 .. K - 1) at a 1000-slot roster spread over 5 rooms, 200 users
    a room, for each colour case and each K, beside the CPU's transducer over the same strings."""
    n = 1000
    cases = []
    for colour in COLOURS:
        with device.Roster(n, look_rooms=len(LOOK_ROOMS)) as roster:
            col = colours(n, colour)
            roster.update(range(n), room=[j % len(LOOK_ROOMS) for j in range(n)], colour=col,
                          name=[b"User%d" % j for j in range(n)], desc=[b"is user %d" % j for j in range(n)])
            ids = list(range(len(LOOK_ROOMS)))
            roster.set_rooms(ids, name=list(LOOK_ROOMS), links=[[(i + 1) % len(ids)] for i in ids], mesg_cnt=ids,
                             desc=[b"The %s.\nA second line of description.\n" % r for r in LOOK_ROOMS],
                             topic=[b"the topic of room %d" % i for i in ids])
            for k in ks:
                slots = [j % n for j in range(k)]
                strings = [look_strings(n, j) for j in slots]
                first = roster.look_many(slots)
                for i, j in enumerate(slots):
                    want = [ch for text in strings[i] for ch in nuts_path.chunks(text, int(col[j]))]
                    if first.chunks(i) != want:
                        raise SystemExit(f"devpath: look {k}, {colour}: look {i} differs from the CPU's transducer over look()'s strings")

                def cpu():
                    for q, j in enumerate(slots):
                        c = int(col[j])
                        for text in strings[q]:
                            nuts_path.chunks(text, c)
                cases.append({"n": n, "k": k, "colour": colour, "rooms": len({j % len(LOOK_ROOMS) for j in slots}),
                              "members": sum(len(x) - 7 for x in strings if len(x) > 7),
                              **_listing_fields(f"look {k}, {colour}", "look", lambda: roster.look_many(slots), cpu, first, k,
                                                reps, warmup)})
    return {"look_kernels": ["nuts_roster_look", "nuts_roster_speak_plan"],
            "look_end_to_end_covers": "packing the K lookers into pinned memory, one H2D (the table, the speaker state, the "
                                      "room table and the descriptions only in a call after an update of theirs), two "
                                      "kernels -- the rooms' texts, a line per user of those rooms, every looker's member "
                                      "list; then both variants of every text --, one D2H at the bound size, one "
                                      "synchronise (python_us adds checking the lookers, counting the rooms' slots, the "
                                      "copies out of pinned memory and building the Look; Look.chunks() is not timed)",
            "look_cpu_us_covers": "np_write_user_stream of the CPU restatement (nuts_path, through ctypes, a call per "
                                  "string) over the strings look() composes for the K lookers, composed beforehand: this "
                                  "leaves the CPU's composing out -- the sprintf calls and the walk over the user list "
                                  "-- and includes a ctypes call per string",
            "look": cases}


WHO_NOW, WHO_DATE = 1_000_000, b"on Monday 19 October 2026 at 00:07"
_COLCOM = (b"RS", b"OL", b"UL", b"LI", b"RV", b"FK", b"FR", b"FG", b"FY", b"FB", b"FM", b"FT", b"FW", b"BK", b"BR", b"BG", b"BY",
           b"BB", b"BM", b"BT", b"BW")


def colour_com_count(s: bytes) -> int:
    """colour_com_count (nuts333.c:2563-2583): behind a ``~`` the table is walked once; a match counts, advances one byte
    and lets the walk go on with the entries after it at the new place."""
    at, cnt = 0, 0
    while at < len(s):
        at += 1
        if s[at - 1] == 0x7e:
            for code in _COLCOM:
                if s[at:at + 2] == code:
                    cnt += 1
                    at += 1
    return cnt


def who_strings(n: int, slot: int) -> list[bytes]:
    """What who(user, 0) hands to write_user for ``slot`` of the roster ``who_cases`` builds: n users spread over the five
    rooms, slot j in room j % 5 and logged in at second 60 j, every one visible, a USER and not AFK."""
    out = [b"\n~BB*** Current users %s ***\n\n" % WHO_DATE]
    for j in range(n):
        line = b"  User%d is user %d~RS" % (j, j)
        out.append(b"%-*s : %-4s : %-12s : %d mins.\n" % (40 + 3 * colour_com_count(line), line, b"USER", LOOK_ROOMS[j % len(LOOK_ROOMS)],
                                                         (WHO_NOW - 60 * j) // 60))
    return out + [b"\nThere are %d visible, 0 invisible, 0 remote users.\nTotal of %d users" % (n, n), b".\n\n"]


def who_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``who`` section: who_many of K lookers (slots 0 .. K - 1) at a 1000-slot roster over LOOK_ROOMS, for each colour
    case and each K, beside the CPU composing the same strings and transducing them."""
    n = 1000
    cases = []
    for colour in COLOURS:
        with device.Roster(n, look_rooms=len(LOOK_ROOMS)) as roster:
            col = colours(n, colour)
            roster.update(range(n), room=[j % len(LOOK_ROOMS) for j in range(n)], colour=col, name=[b"User%d" % j for j in range(n)],
                          desc=[b"is user %d" % j for j in range(n)], last_login=[60 * j for j in range(n)], level=1)
            roster.set_rooms(list(range(len(LOOK_ROOMS))), name=list(LOOK_ROOMS))
            for k in ks:
                slots = [j % n for j in range(k)]
                first = roster.who_many(slots, now=WHO_NOW, date=WHO_DATE)
                for i, j in enumerate(slots):
                    want = [ch for text in who_strings(n, j) for ch in nuts_path.chunks(text, int(col[j]))]
                    if first.chunks(i) != want:
                        raise SystemExit(f"devpath: who {k}, {colour}: who {i} differs from the CPU's transducer over who()'s strings")

                def cpu():
                    for j in slots:
                        c = int(col[j])
                        for text in who_strings(n, j):
                            nuts_path.chunks(text, c)
                cases.append({"n": n, "k": k, "colour": colour, "lines": len(first.line_slots),
                              **_listing_fields(f"who {k}, {colour}", "who",
                                                lambda: roster.who_many(slots, now=WHO_NOW, date=WHO_DATE), cpu, first, k,
                                                reps, warmup)})
    return {"who_kernels": list(device.WHO_KERNELS) + ["nuts_roster_speak_plan"],
            "who_end_to_end_covers": "packing the K lookers and the date into pinned memory, one H2D (the table, the speaker "
                                     "state, the room table, the descriptions and the login times only in a call after an "
                                     "update of theirs), three kernels -- a line per listed user in list order, the headers "
                                     "and the footer; every looker's bitmap of lines; then both variants of every text --, "
                                     "one D2H at the bound size, one synchronise (python_us adds checking the lookers and the "
                                     "listed users' rooms, the copies out of pinned memory and building the Who; Who.chunks() "
                                     "is not timed)",
            "who_cpu_us_covers": "composing who()'s strings for each of the K lookers in Python (the walk over the user list, "
                                 "colour_com_count and the format of every line: interpreted, far slower than the reference's "
                                 "sprintf calls) and np_write_user_stream of the CPU restatement (nuts_path, through ctypes, a "
                                 "call per string) over them",
            "who": cases}


#: the room lists of the ``rooms`` section: the six rooms of provision.SIX_ROOMS with the shipped accesses, and 1,024 rooms
ROOMS_LISTS = {"6": ([b"drive", b"hallway", b"wizroom", b"corridor", b"lounge", b"shop"],
                     [device.FIXED_PUBLIC, device.FIXED_PUBLIC, device.FIXED_PRIVATE, device.PUBLIC, device.PUBLIC, device.PUBLIC]),
               "1024": ([b"room%04d" % i for i in range(device.MAX_LOOK_ROOMS)], [i % 4 for i in range(device.MAX_LOOK_ROOMS)])}
ROOMS_HEADS = {True: b"\n~BB*** Rooms data ***\n\n~FTRoom name            : Access  Users  Mesgs  Topic\n\n",
               False: b"\n~BB*** Rooms data ***\n\n~FTRoom name            : Access  Users  Mesgs  Inlink  LStat  Service\n\n"}


def rooms_strings(n: int, which: str, topics: bool) -> list[bytes]:
    """What rooms(user, show_topics) hands to write_user at the roster ``rooms_cases`` builds: n users, slot j in room
    j % R of the R rooms of ROOMS_LISTS[which]; room i has i messages and the topic ``the topic of room i``, every third
    room an inlink, every fifth a netlink to ``service<i>`` in state i % 3."""
    names, accesses = ROOMS_LISTS[which]
    stats = (b"~FRDOWN", b" ~FYVER", b"  ~FGUP")
    out = [ROOMS_HEADS[topics]]
    for i, (name, access) in enumerate(zip(names, accesses)):
        word = bytearray(b" ~FRPRIV" if access & 1 else b"  ~FGPUB")
        if access & 2:
            word[0] = 0x2a
        count = len(range(i, n, len(names)))
        if topics:
            out.append(b"%-20s : %9s~RS    %3d    %3d  %s\n" % (name, bytes(word), count, i, b"the topic of room %d" % i))
        else:
            inlink, linked = i % 3 == 0, i % 5 == 0
            stat = stats[i % 3] if linked else b"~FRDOWN" if inlink else b"   -"
            out.append(b"%-20s : %9s~RS    %3d    %3d     %s   %s~RS  %s\n" % (name, bytes(word), count, i, b"YES" if inlink else b" NO",
                                                                               stat, b"service%d" % i if linked else b""))
    return out + [b"\n"]


def rooms_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``rooms`` section: rooms_many of K lookers (slots 0 .. K - 1) of one kind at a 1000-slot roster, over the 6
    default rooms and over 1,024 rooms, for each kind, each colour case and each K, beside the CPU composing the same
    strings and transducing them."""
    n = 1000
    cases = []
    for which, (names, accesses) in ROOMS_LISTS.items():
        nr = len(names)
        for colour in COLOURS:
            with device.Roster(n, look_rooms=nr) as roster:
                col = colours(n, colour)
                roster.update(range(n), room=[j % nr for j in range(n)], colour=col, name=[b"User%d" % j for j in range(n)])
                ids = list(range(nr))
                roster.set_rooms(ids, name=names, access=accesses, mesg_cnt=ids, topic=[b"the topic of room %d" % i for i in ids],
                                 inlink=[i % 3 == 0 for i in ids],
                                 netlink=[(b"service%d" % i, False, i % 3) if i % 5 == 0 else None for i in ids])
                for topics in (True, False):
                    for k in ks:
                        slots = [j % n for j in range(k)]
                        first = roster.rooms_many(slots, topics=topics)
                        for i, j in enumerate(slots):
                            want = [ch for text in rooms_strings(n, which, topics) for ch in nuts_path.chunks(text, int(col[j]))]
                            if first.chunks(i) != want:
                                raise SystemExit(f"devpath: rooms {k}, {which} rooms, {colour}: looker {i} differs from the CPU's "
                                                 f"transducer over rooms()'s strings")

                        def cpu():
                            for j in slots:
                                c = int(col[j])
                                for text in rooms_strings(n, which, topics):
                                    nuts_path.chunks(text, c)
                        cases.append({"n": n, "k": k, "colour": colour, "rooms": nr, "kind": "rmst" if topics else "rmsn",
                                      **_listing_fields(f"rooms {k}, {which} rooms, {colour}", "rooms",
                                                        lambda: roster.rooms_many(slots, topics=topics), cpu, first, k,
                                                        reps, warmup)})
    return {"rooms_kernels": list(device.ROOMS_KERNELS) + ["nuts_roster_speak_plan"],
            "rooms_end_to_end_covers": "packing the K lookers into pinned memory, one H2D (the table, the speaker state and the "
                                       "room table only in a call after an update of theirs), a memset of the counters and "
                                       "three kernels -- the users of every room counted over the whole roster; a line of the "
                                       "kind asked for per room, the header and the tail; then both variants of every text --, "
                                       "one D2H at the bound size, one synchronise (python_us adds checking the lookers, the "
                                       "copies out of pinned memory and building the Rooms; Rooms.chunks() is not timed)",
            "rooms_cpu_us_covers": "composing rooms()'s strings for each of the K lookers in Python (the count of every room in "
                                   "closed form, not the reference's walk over the user list per room, and the format of every "
                                   "line: interpreted, slower than the reference's sprintf calls) and np_write_user_stream of the "
                                   "CPU restatement (nuts_path, through ctypes, a call per string) over them",
            "rooms": cases}


#: the six default rooms' links (provision.SIX_ROOMS): the hallway joins the drive, the corridor, the wizroom and the shop
GO_LINKS = ([1], [0, 3, 2, 5], [1], [1, 4], [3], [1])
#: where a mover standing in room r walks to, and back from: a room that adjoins r both ways
GO_THERE = (1, 0, 1, 4, 3, 1)
_ACCESS_WORDS = {device.PUBLIC: b"set to ~FGPUBLIC~RS", device.FIXED_PUBLIC: b"~FRfixed~RS to ~FGPUBLIC~RS",
                 device.FIXED_PRIVATE: b"~FRfixed~RS to ~FRPRIVATE~RS"}


class _Visits(NamedTuple):
    """The device visits of one step, their timings added up: what ``_timed`` reads of a result."""
    timing: dict


def _visits(*results) -> _Visits:
    total = {}
    for r in results:
        for f, v in (r.timing if r is not None else {}).items():
            total[f] = total.get(f, 0) + v
    return _Visits(total)


def go_look_strings(room_of: np.ndarray, slot: int) -> list[bytes]:
    """What look() hands to write_user for ``slot`` of the roster ``go_cases`` builds, its users standing in ``room_of``:
    every user visible, of one level, without a description, no topic and no message anywhere."""
    names, accesses = ROOMS_LISTS["6"]
    rm = int(room_of[slot])
    col = lambda r: b"~FR" if accesses[r] & 1 else b"~FG"
    lines = [b"      User%d ~RS  \n" % j for j in np.flatnonzero(room_of == rm).tolist() if j != slot]
    return ([b"\n~FTRoom: %s%s\n\n" % (col(rm), names[rm]), b"",
             b"\n~FTExits are:" + b"".join(b"  %s%s" % (col(l), names[l]) for l in GO_LINKS[rm]) + b"\n\n"]
            + ([b"~FTYou can see:\n"] + lines if lines else [b"~FTYou are all alone here.\n"])
            + [b"\n", b"Access is %s and there are ~OL~FM0~RS messages on the board.\n" % _ACCESS_WORDS[accesses[rm]],
               b"No topic has been set yet.\n"])


def go_model(room_of: np.ndarray, events) -> list[tuple]:
    """What go_many answers for ``events`` at that roster, where every user is a visible WIZ and no room is exactly PRIVATE:
    per event ``(outcome, target, enter line, leave line, reply)``.  The moves are applied to ``room_of``."""
    names = ROOMS_LISTS["6"][0]
    slots, rooms, out = set(), set(), []
    for slot, word, _wc in events:
        here, target = int(room_of[slot]), names.index(word)
        if slot in slots or here in rooms or target in rooms:
            out.append((device.GO_DEFERRED, target, None, None, None))
        elif target == here:
            out.append((device.GO_ALREADY, target, None, None, b"You are already in the %s!\n" % word))
        else:
            out.append((device.GO_WALKED, target, b"User%d enters.\n" % slot, b"User%d goes to the %s.\n" % (slot, word), None))
            slots.add(slot)
            rooms |= {here, target}
            room_of[slot] = target
    return out


def go_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``go`` section: go_many of K walks (slots 0 .. K - 1) at a 1000-slot roster over the six default rooms, there in
    one call and back in the next, so that the state is periodic; beside the parts a go_many call is made of --
    plan_many of the same composed lines, then look_many of the same movers -- and the CPU composing the strings in
    Python and transducing them."""
    n = 1000
    names, accesses = ROOMS_LISTS["6"]
    nr = len(names)
    cases = []
    for colour in COLOURS:
        with device.Roster(n, look_rooms=nr) as roster:
            col = colours(n, colour)
            home = np.arange(n) % nr
            roster.update(range(n), room=home.tolist(), colour=col, name=[b"User%d" % j for j in range(n)], level=2)
            roster.set_rooms(list(range(nr)), name=names, access=accesses, links=[list(l) for l in GO_LINKS])
            settings = {"gatecrash_level": 3, "min_private_users": 2}
            for k in ks:
                movers = [j % n for j in range(k)]
                there = [(j, names[GO_THERE[int(home[j])]], 2) for j in movers]
                back = [(j, names[int(home[j])], 2) for j in movers]
                room_of = home.copy()
                want_there = go_model(room_of, there)
                moved = [j for j, w in zip(movers, want_there) if w[0] == device.GO_WALKED]
                looks = {j: go_look_strings(room_of, j) for j in moved}
                first = roster.go_many(there, **settings)
                if first.outcome.tolist() != [w[0] for w in want_there] or first.target.tolist() != [w[1] for w in want_there]:
                    raise SystemExit(f"devpath: go {k}, {colour}: the device's outcomes differ from the model's")
                for i, w in enumerate(want_there):
                    if (first.enter_text(i), first.leave_text(i), first.reply_text(i)) != tuple(x or b"" for x in w[2:]):
                        raise SystemExit(f"devpath: go {k}, {colour}: event {i}'s texts differ from the reference's formats")
                for i, j in enumerate(moved):
                    if first.look.chunks(i) != [ch for text in looks[j] for ch in nuts_path.chunks(text, int(col[j]))]:
                        raise SystemExit(f"devpath: go {k}, {colour}: look {i} differs from the CPU's transducer over look()'s strings")
                want_back = go_model(room_of, back)
                second = roster.go_many(back, **settings)
                if second.outcome.tolist() != [w[0] for w in want_back] or not np.array_equal(room_of, home) or not np.array_equal(roster._room, home):
                    raise SystemExit(f"devpath: go {k}, {colour}: the walk back does not end where the walk there began")
                lines = [(w[2], w[1], None, 0, device.COM_GO) for w in want_there if w[2]]
                lines += [(w[3], int(home[j]), j, 0, device.COM_GO) for j, w in zip(movers, want_there) if w[3]]
                lines += [(w[4], None, None, 0, device.COM_GO) for w in want_there if w[4]]

                def parts():
                    return _visits(roster.plan_many(lines) if lines else None, roster.look_many(moved) if moved else None)

                def cpu():
                    rooms = home.copy()
                    for j, w in zip(movers, go_model(rooms, there)):
                        for text in w[2:]:
                            if text:
                                nuts_path.chunks(text, 0)
                                nuts_path.chunks(text, 1)
                        if w[0] == device.GO_WALKED:
                            c = int(col[j])
                            for text in go_look_strings(rooms, j):
                                nuts_path.chunks(text, c)

                def go(events):
                    g = roster.go_many(events, **settings)
                    return _visits(g, g.look)

                timed = _timed(f"go {k}, {colour}", {"there": lambda: go(there), "back": lambda: go(back), "parts": parts, "cpu": cpu},
                               reps, warmup)
                dev, cpu_us = timed["there"], timed["cpu"].host_us
                count = lambda want, what: sum(w[0] == what for w in want)
                cases.append({"n": n, "k": k, "colour": colour, "rooms": nr, "moved": len(moved),
                              "deferred": count(want_there, device.GO_DEFERRED), "already": count(want_there, device.GO_ALREADY),
                              "back_moved": count(want_back, device.GO_WALKED), "back_already": count(want_back, device.GO_ALREADY),
                              "back_deferred": count(want_back, device.GO_DEFERRED),
                              "bytes_out": sum(len(first.look.output(i)) for i in range(len(moved))), **dev.fields, "cpu_us": cpu_us,
                              "back": timed["back"].fields, "parts": timed["parts"].fields,
                              "go_over_parts": {f: round(dev.times[f]["median"] / timed["parts"].times[f]["median"], 2) for f in FIELDS},
                              "end_to_end_over_cpu": float(f"{dev.times['end_to_end_us']['median'] / cpu_us['median']:.3g}")})
    return {"go_kernels": list(device.GO_KERNELS) + ["nuts_roster_speak_plan", "nuts_roster_look", "nuts_roster_speak_plan"],
            "go_end_to_end_covers": "both device visits of a go_many call, added up.  The first: packing the K events into pinned "
                                    "memory, one H2D (the events alone: the look of the call before left every mirror clean), "
                                    "three kernels -- get_room, the decision chain, the texts; the deferral walk; both variants "
                                    "of every text and the room lines' admit bitmaps --, one D2H at the bound size, one "
                                    "synchronise.  Between the visits the binding applies the moves to the host mirrors.  The "
                                    "second: look_many of the movers, which uploads the table the moves made stale, 5 bytes a "
                                    "slot (python_us adds checking the events, the copies out of pinned memory, the applying "
                                    "and building the Go)",
            "go_parts_covers": "plan_many of the lines the same call composes, composed beforehand, then look_many of the same "
                               "movers, at a roster nobody moved in: neither uploads the table",
            "go_cpu_us_covers": "the model of the call in Python -- the deferral rule and the reference's formats, interpreted --, "
                                "np_write_user_stream of the CPU restatement (nuts_path, through ctypes) over both variants of "
                                "every line, and look()'s strings composed in Python for every mover and transduced for its colour",
            "go": cases}


_ACCESS_TO = {device.COM_PRIVATE: (b"~FRPRIVATE", device.PRIVATE, device.ACCESS_SET_PRIVATE, device.ACCESS_ALREADY_PRIVATE, b"private"),
              device.COM_PUBLIC: (b"~FGPUBLIC", device.PUBLIC, device.ACCESS_SET_PUBLIC, device.ACCESS_ALREADY_PUBLIC, b"public")}


def access_actors(k: int, n: int) -> list[int]:
    """The actors of ``access_cases``: slot 3 + j stands in room (3 + j) % 6, so the first three stand in the rooms that can
    be set -- the corridor, the lounge, the shop -- the next three in the fixed ones, and the seventh in the corridor again."""
    return [(3 + j) % n for j in range(k)]


def access_model(accesses: list, room_of: np.ndarray, events) -> list[tuple]:
    """What access_many answers for ``.private`` and ``.public`` events without a word at the roster ``access_cases`` builds,
    where every room holds more users than ``min_private_users``: per event ``(outcome, room, reply, here line)``.  The
    changes are applied to ``accesses``."""
    touched, out = set(), []
    for slot, com, _inpstr, _wc in events:
        rm = int(room_of[slot])
        word, to, done, already, name = _ACCESS_TO[com]
        if rm in touched:
            out.append((device.ACCESS_DEFERRED, rm, None, None))
        elif accesses[rm] > device.PRIVATE:
            out.append((device.ACCESS_FIXED, rm, b"This room's access is fixed.\n", None))
        elif accesses[rm] == to:
            out.append((already, rm, b"This room is already %s.\n" % name, None))
        else:
            out.append((done, rm, b"Room set to %s.\n" % word, b"User%d has set the room to %s.\n" % (slot, word)))
            accesses[rm] = to
            touched.add(rm)
    return out


def access_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``access`` section: access_many of K ``.private`` events (``access_actors``, each in its own room) at a 1000-slot
    roster over the six default rooms, and of K ``.public`` events by the same actors in the next call, so that the state is
    periodic and every call sets an access; beside plan_many of the lines the ``.private`` call composes, composed
    beforehand, and the CPU modelling the call in Python and transducing the lines."""
    n = 1000
    names, accesses = ROOMS_LISTS["6"]
    nr = len(names)
    cases = []
    for colour in COLOURS:
        with device.Roster(n, look_rooms=nr) as roster:
            col = colours(n, colour)
            room_of = np.arange(n) % nr
            roster.update(range(n), room=room_of.tolist(), colour=col, name=[b"User%d" % j for j in range(n)], level=1)
            roster.set_rooms(list(range(nr)), name=names, access=accesses, links=[list(l) for l in GO_LINKS])
            settings = {"gatecrash_level": 3, "min_private_users": 2, "ignore_mp_level": 2}
            for k in ks:
                actors = access_actors(k, n)
                private = [(j, device.COM_PRIVATE, b"", 1) for j in actors]
                public = [(j, device.COM_PUBLIC, b"", 1) for j in actors]
                state = list(accesses)
                want_private = access_model(state, room_of, private)
                first = roster.access_many(private, **settings)
                want_public = access_model(state, room_of, public)
                second = roster.access_many(public, **settings)
                for label, got, want in (("private", first, want_private), ("public", second, want_public)):
                    if got.outcome.tolist() != [w[0] for w in want] or any(
                            got.target_room[i] != w[1] for i, w in enumerate(want) if w[0] != device.ACCESS_DEFERRED):
                        raise SystemExit(f"devpath: access {k}, {colour}: the device's outcomes of the .{label} call differ from the model's")
                    for i, w in enumerate(want):
                        if (got.reply_text(i), got.here_text(i)) != tuple(x or b"" for x in w[2:]):
                            raise SystemExit(f"devpath: access {k}, {colour}: event {i}'s texts differ from the reference's formats")
                        j = actors[i]
                        if w[3] and got.here.chunks(i, int(col[j])) != nuts_path.chunks(w[3], int(col[j])):
                            raise SystemExit(f"devpath: access {k}, {colour}: event {i}'s line differs from the CPU's transducer")
                if state != list(accesses) or roster._room_rec[:nr, 21].tolist() != list(accesses):
                    raise SystemExit(f"devpath: access {k}, {colour}: the .public call does not end where the .private call began")
                lines = [(w[3], w[1], j, 0, device.COM_PRIVATE) for j, w in zip(actors, want_private) if w[3]]
                lines += [(w[2], None, None, 0, device.COM_PRIVATE) for w in want_private if w[2]]

                def cpu():
                    for w in access_model(list(accesses), room_of, private):
                        for text in w[2:]:
                            if text:
                                nuts_path.chunks(text, 0)
                                nuts_path.chunks(text, 1)

                timed = _timed(f"access {k}, {colour}", {"private": lambda: roster.access_many(private, **settings),
                                                         "public": lambda: roster.access_many(public, **settings),
                                                         "plan": lambda: roster.plan_many(lines), "cpu": cpu}, reps, warmup)
                dev, cpu_us = timed["private"], timed["cpu"].host_us
                count = lambda want, whats: sum(w[0] in whats for w in want)
                sets = (device.ACCESS_SET_PRIVATE, device.ACCESS_SET_PUBLIC)
                refusals = (device.ACCESS_FIXED, device.ACCESS_ALREADY_PRIVATE, device.ACCESS_ALREADY_PUBLIC)
                cases.append({"n": n, "k": k, "colour": colour, "rooms": nr, "set": count(want_private, sets),
                              "refused": count(want_private, refusals), "deferred": count(want_private, (device.ACCESS_DEFERRED,)),
                              "public_set": count(want_public, sets), "public_refused": count(want_public, refusals),
                              "public_deferred": count(want_public, (device.ACCESS_DEFERRED,)), "lines": len(lines),
                              **dev.fields, "cpu_us": cpu_us, "public": timed["public"].fields, "plan": timed["plan"].fields,
                              "access_over_plan": {f: round(dev.times[f]["median"] / timed["plan"].times[f]["median"], 2) for f in FIELDS},
                              "end_to_end_over_cpu": float(f"{dev.times['end_to_end_us']['median'] / cpu_us['median']:.3g}")})
    return {"access_kernels": list(device.ACCESS_KERNELS) + ["nuts_roster_speak_plan"],
            "access_end_to_end_covers": "packing the K events into pinned memory, one H2D (the events, and the room table, which "
                                        "the call before changed: 1,072 bytes a room), three kernels -- get_room, get_user or "
                                        "the head-count of the room, the decision chain and the texts; the deferral walk; both "
                                        "variants of every text and the room lines' admit bitmaps --, one D2H at the bound size, "
                                        "one synchronise (python_us adds checking the events, the copies out of pinned memory, "
                                        "building the Access and applying it to the host mirrors through set_rooms)",
            "access_plan_covers": "plan_many of the lines the .private call composes -- the room lines, then the actors' own -- "
                                  "composed beforehand, at the same roster, in the same rounds; it uploads no table",
            "access_cpu_us_covers": "the model of the .private call in Python -- the deferral rule and the reference's formats, "
                                    "interpreted, without the head-count, which every room of this roster passes -- and "
                                    "np_write_user_stream of the CPU restatement (nuts_path, through ctypes) over both variants "
                                    "of every line",
            "access": cases}


ACT_HALF = 500          # the roster of ``act_cases``: slots below are WIZes, the actors; slots from here on USERs, the targets


def act_model(room_of: np.ndarray, events) -> list[tuple]:
    """What act_many answers for ``.wake <user>`` and ``.move <user> <room>`` events at the roster ``act_cases`` builds, where
    every user is visible, nobody is muzzled or AFK, every actor a WIZ and every target a USER named in full, and no room is
    exactly PRIVATE: per event ``(outcome, target, room, texts)`` with the texts by kind.  The moves are applied to ``room_of``."""
    names = ROOMS_LISTS["6"][0]
    slots, rooms, out = set(), set(), []
    for slot, com, inpstr, _wc in events:
        words = inpstr.split()
        who, here = int(words[0][4:]), int(room_of[slot])
        old = int(room_of[who])
        rm = names.index(words[1]) if com == device.COM_MOVE else here
        if {slot, who} & slots or {here, old, rm} & rooms:
            out.append((device.ACT_DEFERRED, who, rm, {}))
        elif com == device.COM_WAKE:
            out.append((device.ACT_WOKEN, who, rm, {"reply": b"Wake up call sent.\n",
                                                    "notice": b"\07\n~BR*** User%d says: ~OL~LIWAKE UP!!!~RS~BR ***\n\n" % slot}))
        elif rm == old:
            out.append((device.ACT_MOVE_ALREADY, who, rm, {"reply": b"User%d is already in the %s.\n" % (who, names[rm])}))
        else:
            out.append((device.ACT_MOVED, who, rm, {
                "reply": b"~FT~OLYou chant an ancient spell...\n", "here": b"~FT~OLUser%d chants an ancient spell...\n" % slot,
                "notice": b"\n~FT~OLA giant hand grabs you and pulls you into a magical blue vortex!\n",
                "enter": b"~FT~OLUser%d falls out of a magical blue vortex!\n" % who,
                "leave": b"~FT~OLA giant hand grabs User%d who is pulled into a magical blue vortex!\n" % who}))
            slots.add(who)
            rooms |= {old, rm}
            room_of[who] = rm
    return out


def act_lines(room_of: np.ndarray, events, want) -> list[tuple]:
    """The lines of a call as plan_many takes them: the room lines to their rooms, the single-recipient ones to every room."""
    lines = []
    for (slot, com, _i, _w), (_o, who, rm, texts) in zip(events, want):
        for kind, to, sender in (("here", int(room_of[slot]), slot), ("enter", rm, None), ("leave", int(room_of[who]), who),
                                 ("reply", None, None), ("notice", None, None)):
            if texts.get(kind):
                lines.append((texts[kind], to, sender, 0, com))
    return lines


def act_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``act`` section: act_many of K ``.wake`` events, and of K ``.move`` events there in one call and back in the next,
    at a 1000-slot roster over the six default rooms; each beside the parts such a call is made of -- plan_many of the same
    composed lines, then look_many of the moved users -- and the CPU modelling the call and transducing the strings."""
    n = 1000
    names, accesses = ROOMS_LISTS["6"]
    nr = len(names)
    texts_of = lambda a, i: {"here": a.here_text(i), "enter": a.enter_text(i), "leave": a.leave_text(i), "reply": a.reply_text(i),
                             "notice": a.notice_text(i)}
    cases = []
    for colour in COLOURS:
        with device.Roster(n, look_rooms=nr) as roster:
            col = colours(n, colour)
            home = np.arange(n) % nr
            roster.update(range(n), room=home.tolist(), colour=col, name=[b"User%d" % j for j in range(n)],
                          level=[2 if j < ACT_HALF else 1 for j in range(n)])
            roster.set_rooms(list(range(nr)), name=names, access=accesses, links=[list(l) for l in GO_LINKS])
            settings = {"gatecrash_level": 3, "min_private_users": 2}
            for k in ks:
                actors = [j % ACT_HALF for j in range(k)]
                target = lambda j: ACT_HALF + j % ACT_HALF
                wake = [(j, device.COM_WAKE, b"user%d" % target(j), 2) for j in actors]
                there = [(j, device.COM_MOVE, b"user%d %s" % (target(j), names[(int(home[target(j)]) + 1) % nr]), 3) for j in actors]
                back = [(j, device.COM_MOVE, b"user%d %s" % (target(j), names[int(home[target(j)])]), 3) for j in actors]
                room_of = home.copy()
                want_wake = act_model(room_of, wake)
                wake_lines = act_lines(room_of, wake, want_wake)
                there_lines = act_lines(room_of, there, act_model(home.copy(), there))
                want_there = act_model(room_of, there)
                moved = [w[1] for w in want_there if w[0] == device.ACT_MOVED]
                looks = {j: go_look_strings(room_of, j) for j in moved}
                got_wake, got_there = roster.act_many(wake, **settings), roster.act_many(there, **settings)
                want_back = act_model(room_of, back)
                got_back = roster.act_many(back, **settings)
                for label, got, want in (("wake", got_wake, want_wake), ("move", got_there, want_there), ("back", got_back, want_back)):
                    if got.outcome.tolist() != [w[0] for w in want] or any(
                            (got.target_slot[i], got.target_room[i]) != w[1:3] for i, w in enumerate(want) if w[0] != device.ACT_DEFERRED):
                        raise SystemExit(f"devpath: act {k}, {colour}: the device's outcomes of the {label} call differ from the model's")
                    for i, w in enumerate(want):
                        if texts_of(got, i) != {kind: w[3].get(kind, b"") for kind in ("here", "enter", "leave", "reply", "notice")}:
                            raise SystemExit(f"devpath: act {k}, {colour}: event {i}'s texts of the {label} call differ from the reference's formats")
                        c = int(col[w[1]])
                        if w[3].get("notice") and got.notice.chunks(i, c) != nuts_path.chunks(w[3]["notice"], c):
                            raise SystemExit(f"devpath: act {k}, {colour}: event {i}'s notice differs from the CPU's transducer")
                for i, j in enumerate(moved):
                    if got_there.look.chunks(i) != [ch for text in looks[j] for ch in nuts_path.chunks(text, int(col[j]))]:
                        raise SystemExit(f"devpath: act {k}, {colour}: look {i} differs from the CPU's transducer over look()'s strings")
                if not np.array_equal(room_of, home) or not np.array_equal(roster._room, home):
                    raise SystemExit(f"devpath: act {k}, {colour}: the moves back do not end where the moves there began")

                def cpu(events, looking):
                    rooms = home.copy()
                    for w in act_model(rooms, events):
                        for text in w[3].values():
                            nuts_path.chunks(text, 0)
                            nuts_path.chunks(text, 1)
                        if looking and w[0] == device.ACT_MOVED:
                            c = int(col[w[1]])
                            for text in go_look_strings(rooms, w[1]):
                                nuts_path.chunks(text, c)

                def act(events):
                    a = roster.act_many(events, **settings)
                    return _visits(a, a.look)

                timed = _timed(f"act {k}, {colour}", {
                    "wake": lambda: act(wake), "wake_parts": lambda: roster.plan_many(wake_lines), "wake_cpu": lambda: cpu(wake, False),
                    "move": lambda: act(there), "back": lambda: act(back),
                    "move_parts": lambda: _visits(roster.plan_many(there_lines), roster.look_many(moved) if moved else None),
                    "move_cpu": lambda: cpu(there, True)}, reps, warmup)
                count = lambda want, what: sum(w[0] == what for w in want)

                def beside(name):
                    dev, parts, cpu_us = timed[name], timed[name + "_parts"], timed[name + "_cpu"].host_us
                    ratio = lambda f, a, b: round(dev.times[f][a] / parts.times[f][b], 2)
                    return {**dev.fields, "parts": parts.fields, "cpu_us": cpu_us,
                            "over_parts": {f: ratio(f, "median", "median") for f in FIELDS},
                            "over_parts_p10_p90": {f: [ratio(f, "p10", "p90"), ratio(f, "p90", "p10")] for f in FIELDS},
                            "end_to_end_over_cpu": float(f"{dev.times['end_to_end_us']['median'] / cpu_us['median']:.3g}")}

                cases.append({"n": n, "k": k, "colour": colour, "rooms": nr, "woken": count(want_wake, device.ACT_WOKEN),
                              "wake_lines": len(wake_lines), "moved": len(moved), "already": count(want_there, device.ACT_MOVE_ALREADY),
                              "deferred": count(want_there, device.ACT_DEFERRED), "back_moved": count(want_back, device.ACT_MOVED),
                              "back_already": count(want_back, device.ACT_MOVE_ALREADY), "back_deferred": count(want_back, device.ACT_DEFERRED),
                              "move_lines": len(there_lines), "look_bytes_out": sum(len(got_there.look.output(i)) for i in range(len(moved))),
                              "wake": beside("wake"), "move": beside("move"), "back": timed["back"].fields})
    return {"act_kernels": list(device.ACT_KERNELS) + ["nuts_roster_speak_plan", "nuts_roster_look", "nuts_roster_speak_plan"],
            "act_end_to_end_covers": "the device visits of an act_many call, added up.  The first: packing the K events into pinned "
                                     "memory, one H2D (the events; after a call that moved, nothing else: its look left every "
                                     "mirror clean), three kernels -- get_user, get_room, the decision chain and the six texts; "
                                     "the deferral walk; both variants of every text and the room lines' admit bitmaps --, one D2H "
                                     "at the bound size, one synchronise.  A call that moved somebody then applies the moves to the "
                                     "host mirrors and visits again: look_many of the moved users, which uploads the table the moves "
                                     "made stale, 5 bytes a slot (python_us adds checking the events, the copies out of pinned "
                                     "memory, the applying and building the Act)",
            "act_parts_covers": "plan_many of the lines the same call composes, composed beforehand -- the room lines to their "
                                "rooms, the actors' and the targets' own lines as lines to every room --, then, for the moves, "
                                "look_many of the same users, at a roster nobody moved in: neither uploads the table",
            "act_cpu_us_covers": "the model of the call in Python -- the deferral rule and the reference's formats, interpreted, "
                                 "with the names taken as given, no get_user and no get_room --, np_write_user_stream of the CPU "
                                 "restatement (nuts_path, through ctypes) over both variants of every line, and for a move "
                                 "look()'s strings composed in Python for every moved user and transduced for its colour",
            "act": cases}


def clone_csays(k: int, names) -> list[tuple]:
    """K ``.csay`` events by the owners 0 .. K - 1, each through its clone in room ``j % 6``, with the bodies of
    ``speak_events(k)``; and the lines they compose."""
    bodies = [ev[2] for ev in speak_events(k)]
    events = [(j, device.COM_CSAY, names[j % len(names)] + b" " + body, 9) for j, body in enumerate(bodies)]
    return events, [b"Clone of User%d says: %s\n" % (j, body) for j, body in enumerate(bodies)]


def clone_model(room_of: np.ndarray, actors, destroy: bool) -> list[int]:
    """What clone_many answers for ``.clone`` events without a word by ``actors``, who own no clone, at the roster
    ``clone_cases`` builds, and for the ``.destroy`` events by the same actors in the call after it: the first actor of a
    room is answered, the later ones of that room wait."""
    touched, out = set(), []
    for j in actors:
        rm = int(room_of[j])
        out.append(device.CLONE_DEFERRED if rm in touched else device.CLONE_DESTROYED if destroy else device.CLONE_CREATED)
        touched.add(rm)
    return out


def clone_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``clone`` section: clone_many of K ``.csay`` events by K distinct owners at a 1000-slot roster over the six default
    rooms, beside speak_many of the same bodies as says by the same users, in the same rounds, and the CPU composing and
    transducing the lines; and clone_many of K ``.clone`` events, then of K ``.destroy`` events by the same actors, which
    returns the records to their start."""
    n = 1000
    names, accesses = ROOMS_LISTS["6"]
    nr, most = len(names), max(ks)
    cases = []
    for colour in COLOURS:
        with device.Roster(n, look_rooms=nr, clones=2 * most) as roster:
            col = colours(n, colour)
            room_of = np.arange(n) % nr
            roster.update(range(n), room=room_of.tolist(), colour=col, name=[b"User%d" % j for j in range(n)], level=3)
            roster.set_rooms(list(range(nr)), name=names, access=accesses, links=[list(l) for l in GO_LINKS])
            roster.set_clones(list(range(most)), owner=list(range(most)), room=[j % nr for j in range(most)])
            settings = {"max_clones": 2, "gatecrash_level": 3, "min_private_users": 2}
            for k in ks:
                csays, lines = clone_csays(k, names)
                says = [(j, device.COM_SAY, ev[2], 8) for j, ev in enumerate(speak_events(k))]
                actors = list(range(most, most + k))
                clones = [(j, device.COM_CLONE, b"", 1) for j in actors]
                destroys = [(j, device.COM_DESTROY, b"", 1) for j in actors]
                before = roster._clones.copy()
                made, gone = roster.clone_many(clones, **settings), roster.clone_many(destroys, **settings)
                if made.outcome.tolist() != clone_model(room_of, actors, False) or gone.outcome.tolist() != clone_model(room_of, actors, True):
                    raise SystemExit(f"devpath: clone {k}, {colour}: the .clone and the .destroy call differ from the model's")
                if not np.array_equal(roster._clones, before):
                    raise SystemExit(f"devpath: clone {k}, {colour}: the .destroy call does not end where the .clone call began")
                first = roster.clone_many(csays, **settings)           # it uploads the records: the timed .csay calls upload none
                for i, t in enumerate(lines):
                    ok = (first.outcome[i] == device.CLONE_SAID and first.said_text(i) == t and first.record[i] == i
                          and all(first.said.chunks(i, c) == nuts_path.chunks(t, c) for c in (0, 1)))
                    if not ok:
                        raise SystemExit(f"devpath: clone {k}, {colour}: .csay event {i} differs from the reference's format or the "
                                         f"CPU's transducer")

                def cpu():
                    for j, ev in enumerate(says):
                        text = b"Clone of User%d %ss: %s\n" % (j, nuts_path.lib().np_say_verb(ev[2]), ev[2])
                        nuts_path.chunks(text, 0)
                        nuts_path.chunks(text, 1)

                timed = _timed(f"clone {k}, {colour}", {"csay": lambda: roster.clone_many(csays, **settings),
                                                        "speak": lambda: roster.speak_many(says), "cpu": cpu}, reps, warmup)
                roster.set_clones(0, hear=device.CLONE_HEAR_ALL)       # every timed .clone call uploads the records, the first too
                there = _timed(f"clone {k}, {colour}", {"clone": lambda: roster.clone_many(clones, **settings),
                                                        "destroy": lambda: roster.clone_many(destroys, **settings)}, reps, warmup)
                dev, sp, cpu_us = timed["csay"], timed["speak"], timed["cpu"].host_us
                cases.append({"n": n, "k": k, "colour": colour, "rooms": nr, "records": 2 * most, **dev.fields, "speak": sp.fields,
                              "cpu_us": cpu_us,
                              "csay_over_speak": {f: round(dev.times[f]["median"] / sp.times[f]["median"], 2) for f in FIELDS},
                              # the loosest the rounds allow: the one side's p10 over the other's p90, and the other way round
                              "csay_over_speak_p10_p90": {f: [round(dev.times[f]["p10"] / sp.times[f]["p90"], 2),
                                                              round(dev.times[f]["p90"] / sp.times[f]["p10"], 2)] for f in FIELDS},
                              "end_to_end_over_cpu": float(f"{dev.times['end_to_end_us']['median'] / cpu_us['median']:.3g}"),
                              "created": made.outcome.tolist().count(device.CLONE_CREATED),
                              "deferred": made.outcome.tolist().count(device.CLONE_DEFERRED),
                              "clone": there["clone"].fields, "destroy": there["destroy"].fields})
    return {"clone_kernels": list(device.CLONE_KERNELS) + ["nuts_roster_speak_plan"],
            "clone_end_to_end_covers": "packing the K events into pinned memory, one H2D (the events; in the .clone and the "
                                       ".destroy call also the clone records, which the call before changed: 9 bytes a record "
                                       "in three 256-byte slices), three kernels -- get_room, get_user, the two walks of the "
                                       "records, the decision chain and the texts; the deferral walk; both variants of every "
                                       "text and the room lines' admit bitmaps --, one D2H at the bound size, one synchronise "
                                       "(python_us adds checking the events, the copies out of pinned memory, building the Clone "
                                       "and applying it to the host mirrors through set_clones)",
            "clone_speak_covers": "speak_many of the same K bodies as says by the same K users, at the same roster, in the same "
                                  "rounds: two kernels, two texts an event where the .csay call has one of its six",
            "clone_cpu_us_covers": "np_say_verb, the reference's format in Python and np_write_user_stream of the CPU "
                                   "restatement (nuts_path, through ctypes) over both variants of every said line",
            "clone": cases}


def set_events(k: int) -> tuple:
    """K ``.ignall`` events and K ``.desc <text>`` events by the actors 0 .. K - 1, the descriptions the bodies of
    ``speak_events(k)`` cut to USER_DESC_LEN bytes, and K says of the same bodies by the same users."""
    bodies = [ev[2][:device.USER_DESC_LEN].rstrip() for ev in speak_events(k)]
    return ([(j, device.COM_IGNALL, b"", 1) for j in range(k)], [(j, device.COM_DESC, body, 7) for j, body in enumerate(bodies)],
            [(j, device.COM_SAY, body, 7) for j, body in enumerate(bodies)])


def set_model(room_of: np.ndarray, actors, on: bool) -> list[int]:
    """What set_many answers for ``.ignall`` events by ``actors``, one each, at the roster ``set_cases`` builds: the first
    actor of a room toggles -- on in a call, off in the next --, the later ones of that room wait."""
    touched, out = set(), []
    for j in actors:
        rm = int(room_of[j])
        out.append(device.SET_DEFERRED if rm in touched else device.SET_IGNALL_ON if on else device.SET_IGNALL_OFF)
        touched.add(rm)
    return out


def set_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``set`` section: set_many of K ``.ignall`` events by K actors, and of K ``.desc <text>`` events by the same
    actors, at a 1000-slot roster over the six default rooms, each beside speak_many of the same bodies as says by the same
    users, in the same rounds, and the CPU composing and transducing the lines."""
    n = 1000
    names, accesses = ROOMS_LISTS["6"]
    nr = len(names)
    cases = []
    for colour in COLOURS:
        with device.Roster(n, look_rooms=nr) as roster:
            col = colours(n, colour)
            room_of = np.arange(n) % nr
            roster.update(range(n), room=room_of.tolist(), colour=col, name=[b"User%d" % j for j in range(n)], level=1)
            roster.set_rooms(list(range(nr)), name=names, access=accesses, links=[list(l) for l in GO_LINKS])
            for k in ks:
                ignalls, descs, says = set_events(k)
                actors = list(range(k))
                for on in (True, False):                                # two calls: the flags end where they began
                    got = roster.set_many(ignalls)
                    want = set_model(room_of, actors, on)
                    line = b"User%d is now ignoring everyone.\n" if on else b"User%d is listening again.\n"
                    ok = got.outcome.tolist() == want and all(
                        got.here_text(j) == line % j and all(got.here.chunks(j, c) == nuts_path.chunks(line % j, c) for c in (0, 1))
                        for j in actors if want[j] != device.SET_DEFERRED)
                    if not ok:
                        raise SystemExit(f"devpath: set {k}, {colour}: the .ignall call differs from the rule of the call, the "
                                         f"reference's format or the CPU's transducer")
                first = roster.set_many(descs)                         # it leaves the descriptions changed, as every timed call does
                if first.outcome.tolist() != [device.SET_DESC_SET] * k or any(
                        first.reply_text(j) != b"Description set.\n" or bytes(roster._udesc[j, :len(descs[j][2])]) != descs[j][2] for j in actors):
                    raise SystemExit(f"devpath: set {k}, {colour}: the .desc call differs from the reference's format")
                toggled = want.count(device.SET_IGNALL_OFF)

                def cpu_ignall():
                    for j in actors[:toggled]:
                        for text in (b"You are now ignoring everyone.\n", b"User%d is now ignoring everyone.\n" % j):
                            nuts_path.chunks(text, 0)
                            nuts_path.chunks(text, 1)

                def cpu_desc():
                    for _ in actors:
                        nuts_path.chunks(b"Description set.\n", 0)
                        nuts_path.chunks(b"Description set.\n", 1)

                roster.set_many(ignalls)                                # the table is changed: the first timed speak_many uploads it too
                one = _timed(f"set {k}, {colour}", {"speak": lambda: roster.speak_many(says), "ignall": lambda: roster.set_many(ignalls),
                                                    "cpu": cpu_ignall}, reps, warmup)
                roster.set_many(descs)                                  # it takes that table, and leaves the descriptions changed
                two = _timed(f"set {k}, {colour}", {"speak": lambda: roster.speak_many(says), "desc": lambda: roster.set_many(descs),
                                                    "cpu": cpu_desc}, reps, warmup)
                if (warmup + reps) % 2 == 0:                            # an odd count of .ignall calls: once more, back to the start
                    roster.set_many(ignalls)

                def over(dev, sp):
                    return ({f: round(dev.times[f]["median"] / sp.times[f]["median"], 2) for f in FIELDS},
                            # the loosest the rounds allow: the one side's p10 over the other's p90, and the other way round
                            {f: [round(dev.times[f]["p10"] / sp.times[f]["p90"], 2), round(dev.times[f]["p90"] / sp.times[f]["p10"], 2)]
                             for f in FIELDS})

                ig, de = over(one["ignall"], one["speak"]), over(two["desc"], two["speak"])
                cases.append({"n": n, "k": k, "colour": colour, "rooms": nr, "toggled": toggled, "deferred": k - toggled,
                              "ignall": {**one["ignall"].fields, "speak": one["speak"].fields, "cpu_us": one["cpu"].host_us},
                              "ignall_over_speak": ig[0], "ignall_over_speak_p10_p90": ig[1],
                              "desc": {**two["desc"].fields, "speak": two["speak"].fields, "cpu_us": two["cpu"].host_us},
                              "desc_over_speak": de[0], "desc_over_speak_p10_p90": de[1]})
    return {"set_kernels": list(device.SET_KERNELS) + ["nuts_roster_speak_plan"],
            "set_end_to_end_covers": "packing the K events into pinned memory and ranking their actors' rooms, one H2D (the events, "
                                     "and in the .desc call the descriptions the call before changed and the speaker table behind them, 48 bytes a slot; the table "
                                     "an .ignall call changes, 5 bytes a slot, travels with the speak_many that follows it), "
                                     "three kernels -- the decision and the "
                                     "three texts of every event; the deferral walk; both variants of every text and the here "
                                     "lines' admit bitmaps --, one D2H at the bound size, one synchronise (python_us adds checking "
                                     "the events, the copies out of pinned memory, building the Settings and applying it to the "
                                     "host mirrors through update)",
            "set_speak_covers": "speak_many of the same K bodies as says by the same K users, at the same roster, in the same "
                                "rounds: two kernels, two texts an event where the set call has three",
            "set_cpu_us_covers": "the reference's formats in Python and np_write_user_stream of the CPU restatement (nuts_path, "
                                 "through ctypes) over both variants of the lines of the events that are answered",
            "set": cases}


RELAY_CLONES = 64


def relay_broadcasts(k: int) -> list[tuple]:
    """K says of slot 5 to room 0 of the roster ``relay_cases`` builds."""
    return [(b"User5 says: " + body + b"\n", 0, 5, 0, device.COM_SAY) for body in (b"relayed line %06d of the bench" % i for i in range(k))]


def relay_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``relay`` section: relay_many of K says to room 0 of a 1000-slot roster spread over 5 rooms, with 0, 1 and 64 of
    its 64 clone records standing in that room, beside plan_many of the same broadcasts and the CPU doing clone_relay's
    work."""
    n = 1000
    lib = nuts_path.lib()
    cases = []
    for colour in COLOURS:
        col = colours(n, colour)
        for relaying in (0, 1, RELAY_CLONES):
            with device.Roster(n, look_rooms=len(LOOK_ROOMS), clones=RELAY_CLONES) as roster:
                roster.update(range(n), room=[j % len(LOOK_ROOMS) for j in range(n)], colour=col)
                roster.set_rooms(list(range(len(LOOK_ROOMS))), name=list(LOOK_ROOMS))
                owners = [10 + c for c in range(relaying)]              # a clone of slots 10 .. in room 0, hearing all
                if relaying:
                    roster.set_clones(list(range(relaying)), owner=owners, room=0)
                for k in ks:
                    bs = relay_broadcasts(k)
                    texts = [b"~FT[ " + LOOK_ROOMS[0] + b" ]:~RS " + b[0] for b in bs]
                    first = roster.relay_many(bs)
                    for i in range(k):
                        if first.owners(i).tolist() != owners or any(
                                first.relay_chunks(i, c) != (nuts_path.chunks(texts[i], c) if relaying else []) for c in (0, 1)):
                            raise SystemExit(f"devpath: relay {k}, {colour}, {relaying} clones: broadcast {i} differs from the "
                                             f"CPU's transducer over the prefixed text")

                    def cpu():
                        for q in range(k):
                            for o in owners:
                                lib.np_contains_swearing(bs[q][0])
                                nuts_path.chunks(texts[q], int(col[o]))
                    rl, pl, cp = _timed(f"relay {k}, {colour}", {"relay": lambda: roster.relay_many(bs),
                                                                 "plan": lambda: roster.plan_many(bs), "cpu": cpu},
                                        reps, warmup).values()
                    e2e = rl.times["end_to_end_us"]["median"]
                    cases.append({"n": n, "k": k, "colour": colour, "relaying_clones": relaying, "relays": k * relaying,
                                  "relay_bytes_out": sum(len(first.relay_variant(i, int(col[o]))) for i in range(k) for o in owners),
                                  **rl.times, **{f"plan_{f}": v for f, v in pl.times.items()}, "cpu_us": cp.host_us,
                                  **rl.copied, **{f"plan_{f}": v for f, v in pl.copied.items()},
                                  "end_to_end_over_plan": float(f"{e2e / pl.times['end_to_end_us']['median']:.3g}"),
                                  "end_to_end_over_cpu": float(f"{e2e / cp.host_us['median']:.3g}") if relaying else None})
    return {"relay_kernels": list(device.RELAY_KERNELS),
            "relay_end_to_end_covers": "what plan_many's covers -- packing the K inputs into pinned memory, one H2D (the table "
                                       "and the clone records only in a call after an update of theirs, the rooms' names only "
                                       "when one changed), nuts_roster_plan, one D2H at the bound size, one synchronise --, and "
                                       "in the same call the clone senders and the relay texts' offsets in the upload, "
                                       "nuts_roster_relay (the relay bitmap and the relay texts) and nuts_roster_speak_plan "
                                       "over the K relay texts (their variants), and the relay bitmap, texts and variants in "
                                       "the download (python_us adds the checks, the copies out of pinned memory and building "
                                       "the Relay); the plan_ figures are plan_many of the same K broadcasts, timed alternating",
            "relay_cpu_us_covers": "clone_relay's work on the CPU restatement (nuts_path, through ctypes): per broadcast and "
                                   "relaying clone np_contains_swearing of the text and np_write_user_stream of the prefixed "
                                   "text, composed beforehand: this leaves the sprintf and the walk over the user list out, "
                                   "scans for swearing where a clone that hears everything would not, and includes two ctypes "
                                   "calls per relay; with no relaying clone the CPU has nothing to do and the ratio is null",
            "relay": cases}


def _grid(case, ks: list[int], reps: int, warmup: int, pb: dict) -> list[dict]:
    """``case`` for every size, text and colour of the single-broadcast cases and each K."""
    return [case(n, text, colour, k, reps, warmup, pb) for n in SIZES for text in TEXTS for colour in COLOURS for k in ks]


def per_call_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``per_call`` section."""
    return {"per_call_kernels": ["nuts_fanout_measure_many", "rocprim device scan x2", "nuts_fanout_emit_many"],
            "per_call_end_to_end_covers": "packing the K inputs into pinned memory, one H2D, kernels, three D2H, "
                                          "two synchronises (python_us adds building the K tables and the copies "
                                          "out of pinned memory)",
            "per_call": _grid(per_call_case, ks, reps, warmup, pb)}


def roster_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``roster`` section."""
    return {"roster_kernels": ["nuts_roster_measure", "rocprim device scan x2", "nuts_roster_emit"],
            "roster_end_to_end_covers": "packing the K inputs into pinned memory, one H2D (the roster table only in a "
                                        "call after an update: h2d_bytes_first_call), kernels, three D2H, two "
                                        "synchronises (python_us adds checking the K tuples and the copies out of "
                                        "pinned memory)",
            "roster": _grid(roster_case, ks, reps, warmup, pb)}


def plan_cases(ks: list[int], reps: int, warmup: int, pb: dict) -> dict:
    """The ``plan`` section."""
    return {"plan_kernels": ["nuts_roster_plan"],
            "plan_end_to_end_covers": "packing the K inputs into pinned memory, one H2D (the roster table only in a "
                                      "call after an update: h2d_bytes_first_call), one kernel, one D2H of the "
                                      "variants, their chunk sizes and the admit bitmap at their bound size, one "
                                      "synchronise (python_us adds checking the K tuples, the copies out of pinned "
                                      "memory and building the Plan; expand() is not timed)",
            "plan": _grid(plan_case, ks, reps, warmup, pb)}


#: the optional sections, in the order they run and are printed: option, metavar, help, and the name of the function that
#: takes (the option's counts, reps, warmup, pathbench's figures) and returns the section's keys
SECTIONS = (
    ("per-call", "K[,K...]", "also time K broadcasts per broadcast_many call, for each K (the per_call cases)",
     "per_call_cases"),
    ("roster", "K[,K...]", "also time K broadcasts per Roster.broadcast_many call, for each K (the roster cases)",
     "roster_cases"),
    ("plan", "K[,K...]", "also time K broadcasts per Roster.plan_many call, for each K (the plan cases)", "plan_cases"),
    ("review", "Q[,Q...]", "also time Roster.review_many of Q rooms per call, for each Q, and what recording adds to "
                           "plan_many (the review section)", "review_cases"),
    ("speak", "K[,K...]", "also time K say events per Roster.speak_many call, for each K, beside plan_many of the "
                          "same lines composed beforehand (the speak section)", "speak_cases"),
    ("input", "K[,K...]", "also time K raw reads per Roster.input_many call, for each K, beside speak_many of the same "
                          "events parsed beforehand (the input section)", "input_cases"),
    ("tell", "K[,K...]", "also time K tells to one target per Roster.tell_many call, for each K, beside speak_many of K "
                         "says of the same bodies (the tell section)", "tell_cases"),
    ("look", "K[,K...]", "also time K looks per Roster.look_many call at a 1000-slot roster spread over 5 rooms, for each "
                         "K, beside the CPU's transducer over look()'s strings (the look section)", "look_cases"),
    ("relay", "K[,K...]", "also time K says per Roster.relay_many call to a room of a 1000-slot roster with 0, 1 and 64 "
                          "relaying clones in it, for each K, beside plan_many of the same broadcasts and the CPU doing "
                          "clone_relay's work (the relay section)", "relay_cases"),
    ("who", "K[,K...]", "also time K whos per Roster.who_many call at a 1000-slot roster spread over 5 rooms, for each K, "
                        "beside the CPU composing and transducing who()'s strings (the who section)", "who_cases"),
    ("rooms", "K[,K...]", "also time K .rmst and K .rmsn listings per Roster.rooms_many call at a 1000-slot roster over 6 and "
                          "over 1,024 rooms, for each K, beside the CPU composing and transducing rooms()'s strings (the "
                          "rooms section)", "rooms_cases"),
    ("go", "K[,K...]", "also time K walks per Roster.go_many call at a 1000-slot roster over the six default rooms, there and "
                       "back, for each K, beside plan_many and look_many of the same lines and movers and the CPU composing "
                       "and transducing the strings (the go section)", "go_cases"),
    ("access", "K[,K...]", "also time K .private events per Roster.access_many call at a 1000-slot roster over the six default "
                           "rooms, and K .public events in the next, for each K, beside plan_many of the same lines and the CPU "
                           "modelling the call and transducing the lines (the access section)", "access_cases"),
    ("clone", "K[,K...]", "also time K .csay events by K owners per Roster.clone_many call at a 1000-slot roster over the six "
                          "default rooms, for each K, beside speak_many of the same bodies and the CPU composing and transducing "
                          "the lines, and K .clone events, then K .destroy events (the clone section)", "clone_cases"),
    ("set", "K[,K...]", "also time K .ignall events and K .desc events by K actors per Roster.set_many call at a 1000-slot roster "
                        "over the six default rooms, for each K, each beside speak_many of the same bodies and the CPU composing "
                        "and transducing the lines (the set section)", "set_cases"),
    ("act", "K[,K...]", "also time K .wake events and K .move events by K actors per Roster.act_many call at a 1000-slot roster "
                        "over the six default rooms, the moves there and back, for each K, each beside plan_many (and look_many) "
                        "of the same lines and users and the CPU modelling the call and transducing the strings (the act section)",
     "act_cases"),
)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=2000, help="timed broadcasts per case (default 2000)")
    ap.add_argument("--warmup", type=int, default=200, help="untimed broadcasts per case first (default 200)")
    ap.add_argument("--pathbench-iterations", type=int, default=2_000_000)
    # the help lists --who before --relay; the two run, and are printed, the other way round
    for option, metavar, text, _ in sorted(SECTIONS, key=lambda s: SECTIONS.index(s) - 1.5 * (s[0] == "who")):
        ap.add_argument(f"--{option}", type=per_call_counts, default=None, metavar=metavar, help=text)
    a = ap.parse_args(argv)
    if a.reps < 1 or a.warmup < 0:
        ap.error("--reps must be >= 1 and --warmup >= 0")
    if a.review and max(a.review) > device.MAX_REVIEW_ROOMS:
        ap.error(f"argument --review: a roster has at most {device.MAX_REVIEW_ROOMS} review rings")
    if not PATHBENCH.exists():
        nuts_path.build()
    try:
        ngpu = device.device_count()
    except (RuntimeError, OSError, subprocess.SubprocessError) as e:
        print(f"devpath: cannot use the device library: {e}", file=sys.stderr)
        return 2
    if ngpu < 1:
        print("devpath: no GPU visible; this command measures the device path and has no CPU fall-back",
              file=sys.stderr)
        return 2

    t_start = time.perf_counter()
    pb = pathbench(a.pathbench_iterations)
    cases = []
    for n in SIZES:
        for text in TEXTS:
            for colour in COLOURS:
                table = listeners(n, colour)
                run = lambda: device.broadcast(TEXTS[text], table, 0, 0, COM[text])
                first = run()
                expect = sum(len(nuts_path.transduce(TEXTS[text], int(c))) for c in colours(n, colour)[1:])
                if int(first.out_offsets[-1]) != expect or int(first.admitted.sum()) != n - 1:
                    raise SystemExit(f"devpath: {n}/{text}/{colour}: device produced {int(first.out_offsets[-1])} "
                                     f"bytes, the CPU restatement {expect}")
                times = _timed(f"{n}/{text}/{colour}", {"broadcast": run}, a.reps, a.warmup)["broadcast"].times
                cpu = cpu_derived_us(pb, text, colour, n)
                cases.append({"n": n, "text": text, "colour": colour, "recipients": n - 1,
                              "bytes_out": int(first.out_offsets[-1]), "writes": int(first.write_offsets[-1]),
                              "kernels_us": times["kernels_us"], "end_to_end_us": times["end_to_end_us"],
                              "cpu_derived_us": round(cpu, 3),
                              "end_to_end_over_cpu": round(times["end_to_end_us"]["median"] / cpu, 1)})
    sections = {}
    for option, _, _, section in SECTIONS:
        counts = getattr(a, option.replace("-", "_"))
        if counts:
            sections.update(globals()[section](counts, a.reps, a.warmup, pb))      # by name: whatever stands there now
    out = {
        "what": "user-space stage of one broadcast (admit predicate + transducer), device vs CPU",
        "device": "gfx950",
        "kernels": ["nuts_fanout_measure_broadcast", "rocprim device scan x2", "nuts_fanout_emit_broadcast"],
        "reps": a.reps, "warmup": a.warmup,
        "end_to_end_covers": "listener table + text H2D, kernels, admitted/offsets/arena/write-size D2H, synchronise",
        "cpu_derived_from": {"pathbench": {k: v for k, v in pb.items() if k not in ("sink", "admitted")},
                             "formula": "(N-1) x transduce + N x fanout_predicate + format_line_once (derived, not timed)"},
        "cases": cases,
        **sections,
        "wall_s": round(time.perf_counter() - t_start, 1),
    }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
