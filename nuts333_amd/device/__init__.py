"""The user-space stage of a broadcast on the MI355X: ``fanout.hip`` behind a small numpy API.

``broadcast(text, listeners, rm_is_null, force_listen, com_num)`` does for every listener what ``write_room_except`` +
``write_user`` do before ``write(2)`` (nuts333.c:1315-1365, 1410-1415): the admit predicate, then the colour-markup
transducer through the 1000-byte staging buffer.  ``transduce_batch(texts, colours)`` runs the transducer over M
independent items, none filtered.  Both return a :class:`Fanout`: the bytes of item ``i`` are
``arena[out_offsets[i]:out_offsets[i + 1]]`` and its ``write(2)`` chunk sizes are
``write_sizes[write_offsets[i]:write_offsets[i + 1]]`` -- byte-exact and boundary-exact with ``np_write_user_stream``
of the CPU restatement (oracle/nuts_path.c).  An item that is not admitted has no bytes and no chunks.
``broadcast_many(broadcasts)`` does K broadcasts, each what ``broadcast()`` takes, in one device call, with a fixed
number of copies and kernel launches whatever K; its items run broadcast by broadcast (``Fanout.broadcast_offsets``).
:class:`Roster` keeps the talker's listener state (room and flags per slot) on the device between calls; its
``broadcast_many`` takes K ``(text, rm, sender, force_listen, com_num)`` tuples, addressed as ``write_room_except``
addresses them, and the device builds every listener's record, so a call uploads the table only after an update.
``Roster.plan_many`` takes the same tuples and returns a :class:`Plan` instead: per broadcast the two variants a
listener can get (colour off, colour on) with their ``write(2)`` chunk sizes, and one admit bit per slot -- what a talker
needs to ``write(fd, variant[colour], size)`` to every admitted slot, in one kernel, one download and one synchronise.
``Plan.expand()`` replicates it on the host into the :class:`Fanout` that ``Roster.broadcast_many`` returns.
``Roster(capacity, review_rooms=R)`` also keeps the review rings of rooms ``0 .. R - 1`` on the device: what
``record()`` keeps per room (nuts333.c:2062-2070), 15 lines of 202 bytes and a cursor.  ``plan_many(bs, record=...)``
records broadcasts into their rooms' rings as ``say()`` does, planning first; ``Roster.review_many(rooms)`` returns
what ``.review`` sends for each room (nuts333.c:5192-5222, without its header and footer): the non-empty lines, oldest
first, one ``write_user`` each, as a :class:`Review` -- two variants per room with their ``write(2)`` chunk sizes, shaped
like a :class:`Plan`.  ``Roster.clear_review(rooms)`` is ``clear_revbuff``.
``Roster.update(name=, vis=, muzzled=, command_mode=)`` keeps what the speech commands read of a speaker, and
``Roster.speak_many(events)`` does for K ``(slot, com, inpstr, word_count)`` events what ``say()``, ``shout()``,
``emote()`` and ``semote()`` do (nuts333.c:4062-4226): the muzzle, "Say what?" and swearing checks, the verb, the
invisible speaker's name, the two composed texts, and their plans -- a :class:`Speech`.
``Roster.input_many(reads)`` starts one stage earlier, from K ``(slot, data)`` reads of clients in line mode, and does
what ``user_input()`` and ``exec_com()`` do before a command function runs (nuts333.c:136-235, 403-432, 2350-2358,
3753-3831): the read is cut at its first control byte, split into words, the ``; # ! < > -`` shortcuts are mapped, the
command is looked up by prefix in the 92-entry table and checked against the speaker's ``level``
(``Roster.update(level=)``), and the first word is stripped.  It returns an :class:`Input`: per read its ``kind`` (IAC,
EMPTY, REPEAT, UNKNOWN, SPEECH or COMMAND), the command, ``word_count``, the line and ``inpstr`` ranges, and a
``Speech`` of K entries in which every SPEECH read is answered as ``speak_many`` answers it, an UNKNOWN read has the
reply ``Unknown command.`` and every other read is void.  Left to the caller: a REPEAT read (``.`` alone: substitute
the user's stored line and resubmit; with none stored the reference answers ``Unknown command.``), AFK users, users away
over a netlink (rejected, as in ``speak_many``), reads that do not end a line (``get_charclient_line``'s per-user
buffer), the prompt, and every command that is not speech: COMMAND hands back ``com``, ``inpstr`` and ``word_count``.
``Roster.tell_many(events)`` answers the private speech commands among those, ``tell()`` and ``pemote()``
(nuts333.c:4128-4182, 4230-4281), for K ``(slot, com, inpstr, word_count)`` events with ``com`` COM_TELL or COM_PEMOTE:
``get_user()`` (nuts333.c:2362-2379) runs on the device over every slot's name, lowest slot first, then the muzzle, the
AFK / ignall / igntell / offsite checks on the target (``Roster.update(afk=, igntell=, afk_mesg=)``), the verb and the two
composed texts with their plans -- a :class:`Private`.  ``Roster(capacity, revtell=True)`` gives every slot the 5-line
revtell ring of the talker (nuts333.c:7699-7715): ``tell_many(events, record=True)`` stores each told line in its target's
ring, ``Roster.revtell_many(slots)`` returns what ``.revtell`` sends for each slot as a :class:`Review`, and
``Roster.clear_revtell(slots)`` empties rings.
``Roster(capacity, look_rooms=R)`` keeps a room table for rooms ``0 .. R - 1`` on the device (``Roster.set_rooms``:
name, access, description, links, topic, board count, netlink) and every slot's ``desc`` (``Roster.update(desc=)``), and
``Roster.look_many(slots)`` returns what ``look()`` writes for K lookers (nuts333.c:3942-4004) as a :class:`Look`: the
texts of the call -- five per distinct room, three fixed ones, a line per user of those rooms -- with their two
variants, and per looker the users it is shown, in list order.
``Roster(capacity, look_rooms=R, clones=C)`` also keeps C clone records apart from the slots (``Roster.set_clones``: owner,
room, ``clone_hear``), and ``Roster.relay_many(broadcasts)`` answers ``write_room_except`` whole for local users
(nuts333.c:1401-1429): the :class:`Plan` of ``plan_many`` and, per broadcast, which clone records relay it to their owners,
the relay text ``~FT[ <room name> ]:~RS `` + text and its two variants -- a :class:`Relay`.
``Roster.update(last_login=, away=)`` keeps the two fields ``who()`` reads beside those, and ``Roster.who_many(slots, now=,
date=)`` returns what ``.who`` writes for K lookers (nuts333.c:4792-4856, ``people == 0``) as a :class:`Who`: the two headers,
the footer and the tail, a line per listed user with ``colour_com_count``'s padding, and per looker a bitmap of the lines it
is sent.
``Roster.rooms_many(slots, topics=)`` returns what ``.rmst`` and ``.rmsn`` write for K lookers (``rooms()``,
nuts333.c:5661-5700) as a :class:`Rooms`: the header of each kind, the tail and a line of each kind per named look room,
with the users standing in every room counted over the whole roster on the device.  ``Roster.set_rooms(inlink=, netlink=)``
keeps the three netlink facts ``.rmsn`` prints in the room record's flag byte.
``Roster.update(in_phrase=, out_phrase=, invite_room=)`` keeps what ``.go`` reads of a mover beside those, and
``Roster.go_many(events, gatecrash_level=, min_private_users=)`` answers K ``(slot, inpstr, word_count)`` ``.go`` events as
``go()``, ``move_user()`` and ``reset_access()`` do (nuts333.c:4305-4459, 2087-2106) -- a :class:`Go`.  The device decides and
composes: ``get_room``, the adjoined, private and gatecrash checks, the enter, leave and reset lines and the notices, with
their plans.  An event that an earlier move of the same call touched -- its slot, its room or its target -- is deferred and
comes back unanswered, so every answered event is exact against the roster as it was before the call.  The binding applies
the moves to the host mirrors, and the look a move ends with is one ``look_many`` over the movers: at most two device visits.
Left to the caller: the netlink branch (GO_NETLINK), ``.move``, the relay of the three room texts to clones' owners, and the
prompt.
``Roster.access_many(events, gatecrash_level=, min_private_users=, ignore_mp_level=)`` answers what changes the two pieces of
state ``.go`` decides by, a room's ``access`` and a user's ``invite_room``: K ``(slot, com, inpstr, word_count)`` events with
``com`` COM_PUBLIC, COM_PRIVATE, COM_LETMEIN or COM_INVITE, as ``set_room_access()``, ``letmein()`` and ``invite()`` do
(nuts333.c:4543-4693) -- an :class:`Access`.  The device runs ``get_room``, ``get_user`` and the head-count of a room, decides
and composes the actor's line, the two room lines and the invitation, with their plans; an event that an earlier one of the
same call touched is deferred; the binding sets the access and the invitations in the host mirrors.
``Roster.clone_many(events, max_clones=, gatecrash_level=, min_private_users=)`` answers what changes the clone records those
calls read: K ``(slot, com, inpstr, word_count)`` events with ``com`` COM_CLONE, COM_DESTROY, COM_CSAY or COM_CHEAR, as
``create_clone()``, ``destroy_clone()``, ``clone_say()`` and ``clone_hear()`` do (nuts333.c:7100-7210, 7293-7357) -- a
:class:`Clone`.  The device runs ``get_room``, ``get_user``, a walk of the records and the head-count of a room a destroyed
clone leaves, decides and composes the six texts with their plans; an event whose owner or room an earlier one of the same
call touched is deferred; the binding creates, destroys and sets the records in the host mirrors and keeps them in list order.
``Roster.set_many(events)`` answers the third group of commands that change what the other calls read, the fields a user
sets on itself and the topic of its room: K ``(slot, com, inpstr, word_count)`` events with ``com`` one of the fourteen
SET_COMS -- ``.mode``, ``.ignall``, ``.prompt``, ``.desc``, ``.inphr``, ``.outphr``, ``.topic``, ``.vis``, ``.invis``,
``.charecho``, ``.afk``, ``.colour``, ``.ignshout`` and ``.igntell`` -- as the reference's twelve functions do
(nuts333.c:4009, 4463-4539, 4697, 6434, 6881, 7409-7507) -- a :class:`Settings`.  These commands need no ``get_user``, no
``get_room`` and no walk over the roster: a wave per event reads its actor's own rows, decides and composes the actor's two
lines and the room's line, with their plans; an event that an earlier one of the same call touched is deferred; the binding
sets the flags, the texts and the topic in the host mirrors.
``Roster.act_many(events, gatecrash_level=, min_private_users=)`` answers the commands a user aims at another user, ``.move``,
``.wake``, ``.muzzle`` and ``.unmuzzle`` (``move``, ``wake``, ``muzzle`` and ``unmuzzle`` with ``move_user(u, rm, 2)``,
nuts333.c:4726-4768, 6496-6522, 6571-6703, 4409-4459) -- an :class:`Act`.  A block per event runs ``get_user`` over
``word[1]`` and ``get_room`` over ``word[2]``, takes the head-count of a room a moved user leaves, decides and composes the
six texts with their plans; an event whose slots or rooms an earlier one of the same call touched is deferred; the binding
moves the targets, looks for them with one ``look_many`` and keeps ``Roster.update(muzzle_level=)``, the level of a muzzle.

Input is validated before the device is touched (``ValueError``).  The library ``_build/libnuts_device.so`` is built by
``__graft_entry__.build()`` where ``hipcc`` exists, and on demand here when it is missing or older than its source.
There is no CPU fall-back: without a GPU the calls raise ``RuntimeError``.
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SOURCE = HERE / "fanout.hip"
LIBRARY = HERE / "_build" / "libnuts_device.so"

#: NP_TEXT_SIZE (nuts333.h:280): a composed text is at most 1999 bytes
TEXT_SIZE = 2000
#: hard bounds per item, pinned by tests on the CPU restatement: bytes <= 6*len + 4, writes <= MAX_WRITES
MAX_WRITES = 16
#: the columns of a listener record: the six fields of ``struct np_listener`` (oracle/nuts_path.h), then ``colour``
LISTENER_FIELDS = ("login", "has_room", "same_room", "ignall", "ignshout", "is_sender", "colour")
#: NP_NUM_COMMANDS (oracle/nuts_path.h enum np_com)
NUM_COMMANDS = 92
COM_SAY, COM_SHOUT, COM_EMOTE, COM_SEMOTE = 3, 4, 6, 7
#: the private speech commands (NP_TELL, NP_PEMOTE)
COM_TELL, COM_PEMOTE = 5, 8
#: the room listings (NP_RMST, NP_RMSN): ``rooms(user, 1)`` and ``rooms(user, 0)``
COM_RMST, COM_RMSN = 42, 43
#: the kernels of fanout.hip, as rocprofv3 names them (the scans are rocPRIM's)
KERNELS = ("nuts_fanout_measure_broadcast", "nuts_fanout_emit_broadcast",
           "nuts_fanout_measure_batch", "nuts_fanout_emit_batch",
           "nuts_fanout_measure_many", "nuts_fanout_emit_many",
           "nuts_roster_measure", "nuts_roster_emit", "nuts_roster_plan", "nuts_roster_record", "nuts_roster_review",
           "nuts_roster_speak", "nuts_roster_speak_plan", "nuts_roster_parse",
           "nuts_roster_tell", "nuts_roster_record_tell", "nuts_roster_revtell", "nuts_roster_look")
#: the kernel relay_many adds to a plan call (it also runs nuts_roster_plan and, over the relay texts, nuts_roster_speak_plan)
RELAY_KERNELS = ("nuts_roster_relay",)
#: NP_ARR_SIZE (nuts333.h:19): the input line a speech command receives is at most 999 bytes
ARR_SIZE = 1000
#: USER_NAME_LEN (nuts333.h:23) and invisname (nuts333.h:150), the name an invisible speaker is shown by
USER_NAME_LEN, INVISNAME = 12, b"A presence"
#: the talker's word_count is at most MAX_WORDS (nuts333.h:17)
MAX_WORDS = 10
#: what became of a speech event (Speech.outcome): spoken, or one of the three notices to the speaker alone
SPOKEN, MUZZLED, NOTHING, SWEARING = 0, 1, 2, 3
#: what became of a private speech event (Private.outcome): told, MUZZLED, NOTHING, or one of the other notices to the
#: speaker alone -- nobody of that name, oneself, and the four of private_blocked in its order
TOLD, NOBODY, SELF, AFK, IGNALL, IGNTELL, OFFSITE = 0, 4, 5, 6, 7, 8, 9
#: a text composed from ``inpstr`` is at most ``len(inpstr) + COMPOSED_EXTRA`` bytes (pinned by a host test) ...
COMPOSED_EXTRA = 32
#: ... and its slot in a speech call's text buffer is ``len(inpstr) + _SPEAK_SLACK`` wide (kSpeakSlack of fanout.hip):
#: the longest notice, 35 bytes, has to fit beside an empty inpstr
_SPEAK_SLACK = 36
#: a private text composed from ``inpstr`` is at most ``len(inpstr) + PRIVATE_EXTRA`` bytes: a pemote reply to and from
#: 12-byte names over an empty inpstr (strstr finds the empty word in the first name), ``~OL(To `` + 12 + ``)~RS `` + 12 +
#: `` `` + ``\n`` ...
PRIVATE_EXTRA = 38
#: ... and its slot in a private speech call's text buffer is ``len(inpstr) + _TELL_SLACK`` wide (kTellSlack of
#: fanout.hip): the longest notice, a 12-byte name, `` is AFK, message is: ``, 60 bytes of message and a newline, 94 bytes,
#: has to fit beside an empty inpstr (both pinned by a host test)
_TELL_SLACK = 96
#: AFK_MESG_LEN (nuts333.h:25), and a slot's row in the AFK-message mirror: the message padded with zeros, its length
AFK_MESG_LEN, _AFK_ROW = 60, 64
#: the flags byte of a slot's speaker state, as fanout.hip reads it
SPEECH_FLAGS = {"vis": 1, "muzzled": 2, "command_mode": 4, "afk": 8, "igntell": 16}
#: the two bits of that byte only set_many reads (kPrompt, kCharecho of fanout.hip)
SET_FLAGS = {"prompt": 32, "charmode_echo": 64}
#: where a slot's speaker state keeps the speaker's level, and the highest one (enum np_level: NEW 0 .. GOD 4)
_LEVEL_BYTE, MAX_LEVEL = 14, 4
#: what became of a read (Input.kind): a telnet IAC reply, a line without a word, "." alone, a line exec_com answers
#: "Unknown command.", a say / shout / emote / semote, any other command
IAC, EMPTY, REPEAT, UNKNOWN, SPEECH, COMMAND = 0, 1, 2, 3, 4, 5
#: Speech.outcome of an input_many read that no speech command answers
NOT_SPEECH = -1
#: user_input reads at most ARR_SIZE bytes at a time (nuts333.c:142)
READ_SIZE = ARR_SIZE
#: broadcast_many() refuses a call whose arena bound, the sum over its broadcasts of N * max_bytes(len), exceeds this;
#: Roster.plan_many() one whose variant bound, 12 * text bytes + 16 * K, does
MANY_ARENA_CAP = 2 << 30
#: the most slots a Roster holds
MAX_CAPACITY = 65536
#: a room id is None (no room) or an int in [0, ROOM_LIMIT)
ROOM_LIMIT = 2**31 - 1
#: NP_REVIEW_LINES, NP_REVIEW_LEN (oracle/nuts_path.h): a room's review ring is 15 lines of 200 + 2 bytes
REVIEW_LINES, REVIEW_LEN = 15, 200
#: hard bounds of one stored line (at most 201 bytes) through the transducer, pinned by tests on the CPU restatement:
#: 201 newlines with colour on are 6 * 201 + 4 = 1210 bytes in writes of 996, 210 and 4
MAX_LINE_BYTES, MAX_LINE_WRITES = 6 * (REVIEW_LEN + 1) + 4, 3
#: and of one room's review, 15 such lines: 18,150 bytes per variant in 45 writes
MAX_REVIEW_BYTES, MAX_REVIEW_WRITES = REVIEW_LINES * MAX_LINE_BYTES, REVIEW_LINES * MAX_LINE_WRITES
#: a review's variant slot in the download (MAX_REVIEW_BYTES rounded up to 4), as fanout.hip lays it out
_REVIEW_STRIDE = (MAX_REVIEW_BYTES + 3) & ~3
#: the most rooms of a Roster that own a review ring.  A ring is 3,030 bytes, so 1024 of them are 3.1 MB that stay
#: allocated for the roster's life, and a recording call runs one block per ring room, each scanning the call's K
#: rooms and flags: 1024 x K reads, which at K = 1000 is what nuts_roster_plan itself reads of a 1000-slot roster.  It
#: is 32 times the rooms the restated talker can hold (MAX_ROOMS of oracle/talker_port.c), so room enough for a
#: roster that spans many talkers
MAX_REVIEW_ROOMS = 1024
#: NP_REVTELL_LINES: a user's revtell ring is 5 such lines; what ``.revtell`` sends of it is at most 6,050 bytes per
#: variant in 15 writes
REVTELL_LINES = 5
MAX_REVTELL_BYTES, MAX_REVTELL_WRITES = REVTELL_LINES * MAX_LINE_BYTES, REVTELL_LINES * MAX_LINE_WRITES
_REVTELL_STRIDE = (MAX_REVTELL_BYTES + 3) & ~3
#: bit 2 of a broadcast's flags byte: record it (bit 1 is force_listen)
_RECORD_BIT = 4
#: the most rooms of a Roster that own a room record (``Roster(look_rooms=)``): the figure and the reasoning of
#: MAX_REVIEW_ROOMS -- a room's record and description are 1,072 bytes, 1.1 MB at 1024 rooms for the roster's life, and
#: 32 times the rooms the restated talker can hold
MAX_LOOK_ROOMS = 1024
#: ROOM_NAME_LEN, ROOM_DESC_LEN, MAX_LINKS, TOPIC_LEN, SERV_NAME_LEN, USER_DESC_LEN (nuts333.h)
ROOM_NAME_LEN, ROOM_DESC_LEN, MAX_LINKS, TOPIC_LEN, SERV_NAME_LEN, USER_DESC_LEN = 20, 810, 10, 60, 80, 30
#: a room's access (nuts333.h): bit 0 is PRIVATE, bit 1 fixes it
PUBLIC, PRIVATE, FIXED_PUBLIC, FIXED_PRIVATE = 0, 1, 2, 3
#: the room table's rows as fanout.hip reads them (its look section has the fields): a 256-byte record and an 816-byte
#: description row per room, the records first; and a slot's 32-byte row of the users' descriptions
_ROOM_REC, _ROOM_DESC_ROW, _DESC_ROW = 256, 816, 32
#: hard bounds of one member line of look() through the transducer, proven by a host test against the CPU restatement:
#: with colour on its fixed parts give 42 bytes (5 blanks, ~FR, ``*``, ~RS, a blank, ~RS, 2 blanks, ~BR, ``(AFK)``, the
#: newline, the trailing reset) and a byte of name or description at most 6; far below the 994 staged bytes that
#: would flush in mid-line, so it is one write and the reset's
MAX_MEMBER_BYTES, MAX_MEMBER_WRITES = 42 + 6 * (USER_NAME_LEN + USER_DESC_LEN), 2
#: the longest member line before the transducer, and its slot among a look call's texts (kLineRow of fanout.hip)
MAX_MEMBER_LINE, _LINE_ROW = 69, 72
#: a look call's texts (look_text_at, look_fixed_at of fanout.hip): a room's five slots, 1376 bytes in all, are 36, 812, 352,
#: 96 and 80 bytes wide, the longest form of each text; then the three fixed texts in 48 bytes; then the lines
_LOOK_TEXT_AT, _LOOK_STRIDE, _LOOK_FIXED_AT, _LOOK_FIXED_STRIDE = (0, 36, 848, 1200, 1296), 1376, (0, 16, 44), 48
#: the texts of a room in a Look, in look()'s order, and the fixed ones
LOOK_NAME, LOOK_DESC, LOOK_EXITS, LOOK_ACCESS, LOOK_TOPIC = range(5)


#: a clone's ``clone_hear`` (nuts333.h:60-62): it relays nothing, lines that hold a swear word, or everything
CLONE_HEAR_NOTHING, CLONE_HEAR_SWEARS, CLONE_HEAR_ALL = 0, 1, 2
#: the kernels who_many runs before nuts_roster_speak_plan
WHO_KERNELS = ("nuts_roster_who", "nuts_roster_who_shown")
#: a slot's row of the who mirror (kWhoRec of fanout.hip): int32 last_login, int32 away (-1: none)
_WHO_REC = 8
#: the fixed texts of a Who, and the level names ``who()`` prints with %-4s (nuts333.h level_name, without the NONE entry)
WHO_HEAD_LOGIN, WHO_HEAD, WHO_FOOT, WHO_TAIL = range(4)
LEVEL_NAMES = (b"NEW", b"USER", b"WIZ", b"ARCH", b"GOD")
#: long_date()'s buffer is dstr[80]
WHO_DATE_LEN = 79
#: colour_com_count over ``"  " + name + " " + desc + "~RS"`` is at most 25: a count takes a byte of its own and a run a
#: ``~`` before it, and a run is at most three (``~FBBM``), so 12 bytes of name hold 6, 30 of description 18, and ``~RS`` is
#: 1.  The longest line before the transducer is then a first field of 40 + 3 * 25 bytes, `` : ``, 4 of level, `` : ``, ``@``
#: and an 80-byte service, `` : ``, ``-35791394``, `` mins.`` and ``~BR(AFK)\n``: 233 bytes, in a slot of 236 (kWhoRow)
MAX_WHO_COUNT = 25
MAX_WHO_LINE, _WHO_ROW = 40 + 3 * MAX_WHO_COUNT + 3 + 4 + 3 + 1 + SERV_NAME_LEN + 3 + 9 + 6 + 9, 236
#: hard bounds of one who line through the transducer: the transducer's own, 6 bytes for each of its bytes and the reset;
#: and since a write before the last holds at least 995 bytes (the buffer is flushed only past 994), those 1,402 bytes are
#: at most two writes and the reset's
MAX_WHO_LINE_BYTES, MAX_WHO_LINE_WRITES = 6 * MAX_WHO_LINE + 4, 3
#: a who call's texts (who_fixed_at of fanout.hip): the login header and the header in 108 bytes each, the footer in 80,
#: the tail in 8; then the lines
_WHO_FIXED_AT, _WHO_FIXED_STRIDE = (0, 108, 216, 296), 304
#: the kernels rooms_many runs before nuts_roster_speak_plan
ROOMS_KERNELS = ("nuts_roster_rooms_count", "nuts_roster_rooms_lines")
#: a netlink's state as ``rooms()`` tells them apart (nuts333.c:5690-5692): unconnected, connected and not yet up, up
LINK_DOWN, LINK_VERIFYING, LINK_UP = 0, 1, 2
#: the room record's flag byte (byte 24): a netlink that is UP, ``allow == IN``, ``inlink``, a netlink that is unconnected,
#: one that is connected and not up.  A room has a netlink when one of the three state bits is set
_NET_UP, _NET_ALLOW_IN, _NET_INLINK, _NET_DOWN, _NET_VERIFYING = 1, 2, 4, 8, 16
_NET_STATE = {LINK_DOWN: _NET_DOWN, LINK_VERIFYING: _NET_VERIFYING, LINK_UP: _NET_UP}
#: the fixed texts of a Rooms; then ``3 + r`` is room r's ``.rmst`` line and ``3 + look_rooms + r`` its ``.rmsn`` line
ROOMS_HEAD_TOPICS, ROOMS_HEAD_LINKS, ROOMS_TAIL = range(3)
#: the longest lines of ``rooms()`` before the transducer, from its two formats: ``%-20s : %9s~RS    %3d    %3d`` is a
#: 20-byte name, `` : ``, 9 of access, ``~RS`` and four blanks, a count of 65,536 (``%3d`` widens to 5), four blanks and a
#: mesg_cnt of 2^31 - 1 (10); then two blanks, a 60-byte topic and the newline, or five blanks, 3 of inlink, three blanks, 7
#: of stat, ``~RS``, two blanks, an 80-byte service and the newline.  Their slots are kRmstRow and kRmsnRow of fanout.hip
_ROOMS_LINE_FRONT = ROOM_NAME_LEN + 3 + 9 + 3 + 4 + len(str(MAX_CAPACITY)) + 4 + len(str(2**31 - 1))
MAX_RMST_LINE, _RMST_ROW = _ROOMS_LINE_FRONT + 2 + TOPIC_LEN + 1, 124
MAX_RMSN_LINE, _RMSN_ROW = _ROOMS_LINE_FRONT + 5 + 3 + 3 + 7 + 3 + 2 + SERV_NAME_LEN + 1, 164
#: hard bounds of one such line through the transducer, by MAX_WHO_LINE_BYTES' reasoning: the transducer's own 6 bytes per
#: byte and the reset, 730 and 976 bytes; both are below the 995 a flushed write holds, so one write and the reset's
MAX_RMST_LINE_BYTES, MAX_RMSN_LINE_BYTES, MAX_ROOMS_LINE_WRITES = 6 * MAX_RMST_LINE + 4, 6 * MAX_RMSN_LINE + 4, 2
#: a rooms call's texts (rooms_fixed_at of fanout.hip): the two headers in 80 and 96 bytes, the tail in 4; then the
#: ``.rmst`` lines, then the ``.rmsn`` lines
_ROOMS_FIXED_AT, _ROOMS_FIXED_STRIDE = (0, 80, 176), 180
#: ``.go`` (NP_GO), and the kernels go_many runs before nuts_roster_speak_plan
COM_GO = 10
GO_KERNELS = ("nuts_roster_go", "nuts_roster_go_order")
#: what became of a ``.go`` event (Go.outcome).  The first three moved: by a link, by a WIZ's teleport, invisibly.  Then the
#: notices to the mover alone -- "Go where?", no such room, already there, not adjoined, private -- with GO_NETLINK among
#: them, the netlink branch that the caller answers, and GO_DEFERRED, an event the caller submits again
(GO_WALKED, GO_TELEPORTED, GO_UNSEEN, GO_WHERE, GO_NETLINK, GO_NO_ROOM, GO_ALREADY, GO_NOT_ADJOINED, GO_PRIVATE,
 GO_DEFERRED) = range(10)
#: PHRASE_LEN (nuts333.h:26), and a slot's row of the go mirror (kGoRec of fanout.hip): in_phrase padded with zeros and its
#: length at byte 40, out_phrase and its length at bytes 41 .. 81, two zeros, int32 invite_room (-1: none) at byte 84
PHRASE_LEN, _GO_REC, _GO_OUT, _GO_INVITE = 40, 88, 41, 84
#: the longest texts of a move before the transducer (kGoEnterMax .. kGoReplyMax of fanout.hip, pinned by a host test): the
#: teleport's enter line, ``~FT~OL`` + a 12-byte name + 40 bytes; the leave line, a name, a blank, a 40-byte out_phrase,
#: `` to the ``, a 20-byte room name and ``.\n``; the reset line; the not-adjoined notice over a 20-byte room name
MAX_GO_ENTER, MAX_GO_LEAVE, MAX_GO_RESET, MAX_GO_REPLY = (6 + USER_NAME_LEN + 40, USER_NAME_LEN + 1 + PHRASE_LEN + 8 + ROOM_NAME_LEN + 2,
                                                          35, 4 + ROOM_NAME_LEN + 26)
#: their slots among a go call's texts (kGoEnterRow .. kGoReplyRow): with K events the enter lines, then the leave lines,
#: the reset lines and the replies, event k's at ``K x (the rows before) + row x k`` (go_text_at)
_GO_ROWS = (60, 84, 36, 52)
#: the texts of an event in a Go, in that order
GO_ENTER, GO_LEAVE, GO_RESET, GO_REPLY = range(4)
#: ``.public``, ``.private``, ``.letmein`` and ``.invite`` (NP_PUBLIC .. NP_INVITE), and the kernels access_many runs before
#: nuts_roster_speak_plan
COM_PUBLIC, COM_PRIVATE, COM_LETMEIN, COM_INVITE = 16, 17, 18, 19
ACCESS_KERNELS = ("nuts_roster_access", "nuts_roster_access_order")
#: what became of such an event (Access.outcome).  The first three changed something -- a room set private, set public, a
#: user invited -- and ACCESS_ASKED, a ``.letmein`` that was shouted, changed nothing.  Then the refusals to the actor alone,
#: a branch of the reference each: of ``set_room_access`` (level too low for the room option, no such room, access fixed,
#: already public, already private, too few occupants), of ``letmein`` (no word, no such room, already in, not adjoined, the
#: room is public) and of ``invite`` (no word, the room is public, nobody of that name, oneself, already here, already
#: invited); and ACCESS_DEFERRED, an event the caller submits again
(ACCESS_SET_PRIVATE, ACCESS_SET_PUBLIC, ACCESS_INVITED, ACCESS_ASKED, ACCESS_LOW_LEVEL, ACCESS_NO_ROOM, ACCESS_FIXED,
 ACCESS_ALREADY_PUBLIC, ACCESS_ALREADY_PRIVATE, ACCESS_TOO_FEW, ACCESS_LET_WHERE, ACCESS_LET_NO_ROOM, ACCESS_LET_ALREADY,
 ACCESS_LET_NOT_ADJOINED, ACCESS_LET_PUBLIC, ACCESS_INVITE_WHO, ACCESS_INVITE_PUBLIC, ACCESS_INVITE_NOBODY, ACCESS_INVITE_SELF,
 ACCESS_INVITE_HERE, ACCESS_INVITE_ALREADY, ACCESS_DEFERRED) = range(22)
#: the longest texts of such an event before the transducer (kAccHereMax .. kAccNoticeMax of fanout.hip, pinned by a host
#: test): ``letmein``'s line to the asker's room, a 12-byte name, `` shouts asking to be let into the ``, a 20-byte room name
#: and ``.\n``; its line to the other room; the too-few notice with ten digits; the invitation, a name, `` has invited you
#: into the ``, a room name and ``.\n``
MAX_ACCESS_HERE, MAX_ACCESS_THERE, MAX_ACCESS_REPLY, MAX_ACCESS_NOTICE = (USER_NAME_LEN + 34 + ROOM_NAME_LEN + 2, USER_NAME_LEN + 29,
                                                                         18 + 10 + 55, USER_NAME_LEN + 26 + ROOM_NAME_LEN + 2)
#: their slots among an access call's texts (kAccHereRow .. kAccNoticeRow), laid out as _GO_ROWS lays a go call's
_ACCESS_ROWS = (72, 44, 84, 60)
_ACCESS_COMS = (COM_PUBLIC, COM_PRIVATE, COM_LETMEIN, COM_INVITE)
_ACCESS_COM_RULE = f"com must be COM_PUBLIC, COM_PRIVATE, COM_LETMEIN or COM_INVITE ({COM_PUBLIC} .. {COM_INVITE})"
#: the texts of an event in an Access, in that order: the two room lines first, then the two single-recipient texts
ACCESS_HERE, ACCESS_THERE, ACCESS_REPLY, ACCESS_NOTICE = range(4)
#: ``.clone``, ``.destroy``, ``.csay`` and ``.chear`` (NP_CLONE, NP_DESTROY, NP_CSAY, NP_CHEAR), and the kernels clone_many runs
#: before nuts_roster_speak_plan
COM_CLONE, COM_DESTROY, COM_CSAY, COM_CHEAR = 73, 74, 78, 79
CLONE_KERNELS = ("nuts_roster_clone", "nuts_roster_clone_order")
#: what became of such an event (Clone.outcome).  A ``.chear`` that was obeyed has the ``clone_hear`` value it set for its
#: outcome: CLONE_HEAR_NOTHING, CLONE_HEAR_SWEARS or CLONE_HEAR_ALL, 0 .. 2.  Then a clone created, one destroyed and one that
#: spoke; then the refusals to the actor alone, a branch of the reference each and in its order: of ``create_clone`` (no such
#: room, the room is private, already a clone there, the maximum reached), of ``destroy_clone`` (no such room, nobody of that
#: name, the owner's level, no clone of the actor's there, none of the named user's), of ``clone_say`` (muzzled, too few
#: words, no such room, no clone there) and of ``clone_hear`` (usage, no such room, no clone there); and CLONE_DEFERRED, an
#: event the caller submits again
(CLONE_CREATED, CLONE_DESTROYED, CLONE_SAID, CLONE_NO_ROOM, CLONE_PRIVATE, CLONE_ALREADY, CLONE_MAX, CLONE_DESTROY_NO_ROOM,
 CLONE_DESTROY_NOBODY, CLONE_DESTROY_LEVEL, CLONE_DESTROY_NONE_OWN, CLONE_DESTROY_NONE_THEIRS, CLONE_CSAY_MUZZLED, CLONE_CSAY_USAGE,
 CLONE_CSAY_NO_ROOM, CLONE_CSAY_NONE, CLONE_CHEAR_USAGE, CLONE_CHEAR_NO_ROOM, CLONE_CHEAR_NONE, CLONE_DEFERRED) = range(3, 23)
#: the longest of the five short texts of such an event before the transducer (kCloneHereMax .. kCloneNoticeMax of
#: fanout.hip, pinned by a host test), by their format strings: ``~FB~OL``, a 12-byte name and `` whispers a haunting
#: spell...\n``; ``~FB~OLA clone of ``, a name and `` appears in a swirling magical mist!\n``; ``Room access returned to
#: ~FGPUBLIC.\n``; ``~FB~OLYou whisper a haunting spell and a clone is created in the ``, a 20-byte room name and ``.\n``;
#: ``~OLSYSTEM: ~FR``, a name, `` has destroyed your clone in the ``, a room name and ``.\n``
MAX_CLONE_HERE, MAX_CLONE_THERE, MAX_CLONE_RESET, MAX_CLONE_REPLY, MAX_CLONE_NOTICE = (
    6 + USER_NAME_LEN + 30, 17 + USER_NAME_LEN + 37, 35, 65 + ROOM_NAME_LEN + 2, 14 + USER_NAME_LEN + 33 + ROOM_NAME_LEN + 2)
#: their slots among a clone call's texts (kCloneHereRow .. kCloneNoticeRow): each the longest text rounded up to a multiple
#: of 4, in the order above.  The said lines lie between the reset lines and the replies, each in a slot of its inpstr's
#: length and _SPEAK_SLACK, as speak_many lays its composed lines: the texts lie in their own order, room lines first
_CLONE_ROWS = (48, 68, 36, 88, 84)
_CLONE_COMS = (COM_CLONE, COM_DESTROY, COM_CSAY, COM_CHEAR)
_CLONE_COM_RULE = f"com must be COM_CLONE, COM_DESTROY, COM_CSAY or COM_CHEAR ({COM_CLONE}, {COM_DESTROY}, {COM_CSAY}, {COM_CHEAR})"
#: the texts of an event in a Clone, in that order: the four room lines first, then the two single-recipient texts
CLONE_HERE, CLONE_THERE, CLONE_RESET, CLONE_SAID_LINE, CLONE_REPLY, CLONE_NOTICE = range(6)
#: ``.move``, ``.wake``, ``.muzzle`` and ``.unmuzzle`` (NP_MOVE, NP_WAKE, NP_MUZZLE, NP_UNMUZZLE), the commands a user aims at
#: another user, and the kernels act_many runs before nuts_roster_speak_plan
COM_MOVE, COM_WAKE, COM_MUZZLE, COM_UNMUZZLE = 21, 58, 60, 61
ACT_KERNELS = ("nuts_roster_act", "nuts_roster_act_order")
#: what became of such an event (Act.outcome).  The first four changed something -- a user moved, seen or unseen, a muzzle
#: set, a muzzle removed -- and ACT_WOKEN, a wake-up call that was sent, changed nothing.  Then the refusals to the actor
#: alone, a branch of the reference each and in its order: of ``move`` (usage, nobody of that name, no such room, oneself,
#: the target's level, already there, the room is private to the actor, and ACT_MOVE_AWAY, a target that stands in no look
#: room, which the caller answers), of ``wake`` (usage, the actor is muzzled, nobody, oneself, the target is AFK), of
#: ``muzzle`` (usage, ACT_MUZZLE_ABSENT -- nobody of that name is logged on and the reference goes to the user file: the
#: caller's --, oneself, the target's level, already muzzled) and of ``unmuzzle`` (usage, ACT_UNMUZZLE_ABSENT, oneself, not
#: muzzled -- which writes nothing --, a muzzle above the actor's level); and ACT_DEFERRED, an event the caller submits again
(ACT_MOVED, ACT_MOVED_UNSEEN, ACT_MUZZLED, ACT_UNMUZZLED, ACT_WOKEN, ACT_MOVE_USAGE, ACT_MOVE_NOBODY, ACT_MOVE_NO_ROOM, ACT_MOVE_SELF,
 ACT_MOVE_LEVEL, ACT_MOVE_ALREADY, ACT_MOVE_PRIVATE, ACT_MOVE_AWAY, ACT_WAKE_USAGE, ACT_WAKE_MUZZLED, ACT_WAKE_NOBODY, ACT_WAKE_SELF,
 ACT_WAKE_AFK, ACT_MUZZLE_USAGE, ACT_MUZZLE_ABSENT, ACT_MUZZLE_SELF, ACT_MUZZLE_LEVEL, ACT_MUZZLE_ALREADY, ACT_UNMUZZLE_USAGE,
 ACT_UNMUZZLE_ABSENT, ACT_UNMUZZLE_SELF, ACT_UNMUZZLE_NOT, ACT_UNMUZZLE_ABOVE, ACT_DEFERRED) = range(29)
#: the longest texts of such an event before the transducer (kActHereMax .. kActNoticeMax of fanout.hip, pinned by a host
#: test), by their format strings: ``~FT~OL``, a 12-byte name and `` chants an ancient spell...\n``; ``~FT~OL``, a name and
#: `` falls out of a magical blue vortex!\n``; ``~FT~OLA giant hand grabs ``, a name and `` who is pulled into a magical blue
#: vortex!\n``; ``Room access returned to ~FGPUBLIC.\n``; a name, ``'s muzzle is set to level ``, a level's name of at most 4
#: bytes and ``, you do not have the power to remove it.\n``; the giant hand's line to the moved user
MAX_ACT_HERE, MAX_ACT_ENTER, MAX_ACT_LEAVE, MAX_ACT_RESET, MAX_ACT_REPLY, MAX_ACT_NOTICE = (
    6 + USER_NAME_LEN + 28, 6 + USER_NAME_LEN + 37, 25 + USER_NAME_LEN + 43, 35, USER_NAME_LEN + 26 + 4 + 42, 72)
#: their slots among an act call's texts (kActHereRow .. kActNoticeRow): each the longest text rounded up to a multiple of 4,
#: laid out as _GO_ROWS lays a go call's
_ACT_ROWS = (48, 56, 80, 36, 84, 72)
_ACT_COMS = (COM_MOVE, COM_WAKE, COM_MUZZLE, COM_UNMUZZLE)
_ACT_COM_RULE = f"com must be COM_MOVE, COM_WAKE, COM_MUZZLE or COM_UNMUZZLE ({COM_MOVE}, {COM_WAKE}, {COM_MUZZLE}, {COM_UNMUZZLE})"
#: the texts of an event in an Act, in that order: the four room lines first, then the two single-recipient texts
ACT_HERE, ACT_ENTER, ACT_LEAVE, ACT_RESET, ACT_REPLY, ACT_NOTICE = range(6)
#: the muzzle level's byte in a slot's speaker row (kMuzzleByte of fanout.hip), and WIZ, the lowest level that can type
#: ``.muzzle``: the muzzle of a slot whose ``muzzled`` bit is set over a level byte of 0
_MUZZLE_BYTE, LEVEL_WIZ = 15, 2
#: the commands a user sets its own state with (NP_MODE .. NP_IGNTELL of enum np_com), and the kernels set_many runs before
#: nuts_roster_speak_plan
(COM_MODE, COM_IGNALL, COM_PROMPT, COM_DESC, COM_INPHR, COM_OUTPHR, COM_TOPIC, COM_VIS, COM_INVIS, COM_CHARECHO, COM_AFK, COM_COLOUR,
 COM_IGNSHOUT, COM_IGNTELL) = 2, 11, 12, 13, 14, 15, 20, 55, 56, 66, 82, 84, 85, 86
SET_COMS = (COM_MODE, COM_IGNALL, COM_PROMPT, COM_DESC, COM_INPHR, COM_OUTPHR, COM_TOPIC, COM_VIS, COM_INVIS, COM_CHARECHO, COM_AFK,
            COM_COLOUR, COM_IGNSHOUT, COM_IGNTELL)
SET_KERNELS = ("nuts_roster_set", "nuts_roster_set_order")
#: what became of such an event (Settings.outcome), a branch of the reference each.  The first 22 changed something: the
#: toggles by the flag they found -- ``toggle_mode``, ``toggle_ignall``, ``toggle_prompt`` --, a description, an in phrase, an
#: out phrase and a topic set, a user who became visible or invisible, ``toggle_charecho``, AFK and AFK with the session
#: locked, ``toggle_colour``, ``toggle_ignshout`` and ``toggle_igntell``.  Then what changed nothing: the video test of
#: ``toggle_colour``, whose twenty lines are the caller's (COLOUR_TEST); of ``set_desc`` the query, ``(CLONE)`` in the first
#: word and a description too long; of ``set_iophrase`` a phrase too long and the two queries; of ``set_topic`` the query
#: without a topic, the query and a topic too long; already visible, already invisible; an AFK message too long; and
#: SET_DEFERRED, an event the caller submits again
(SET_MODE_COMMAND, SET_MODE_SPEECH, SET_IGNALL_ON, SET_IGNALL_OFF, SET_PROMPT_ON, SET_PROMPT_OFF, SET_DESC_SET, SET_INPHR_SET,
 SET_OUTPHR_SET, SET_TOPIC_SET, SET_VISIBLE, SET_INVISIBLE, SET_CHARECHO_ON, SET_CHARECHO_OFF, SET_AFK, SET_AFK_LOCKED, SET_COLOUR_ON,
 SET_COLOUR_OFF, SET_IGNSHOUT_ON, SET_IGNSHOUT_OFF, SET_IGNTELL_ON, SET_IGNTELL_OFF, SET_COLOUR_TEST, SET_DESC_QUERY, SET_DESC_CLONE,
 SET_DESC_LONG, SET_PHRASE_LONG, SET_INPHR_QUERY, SET_OUTPHR_QUERY, SET_TOPIC_NONE, SET_TOPIC_QUERY, SET_TOPIC_LONG,
 SET_ALREADY_VISIBLE, SET_ALREADY_INVISIBLE, SET_AFK_LONG, SET_DEFERRED) = range(36)
#: the longest texts of such an event before the transducer (kSetHereMax .. kSetReply2Max of fanout.hip, pinned by a host
#: test): a 12-byte name, `` has set the topic to: ``, a 60-byte topic and the newline; ``The current topic is: ``, a topic and
#: the newline; ``AFK message set.\n``
MAX_SET_HERE, MAX_SET_REPLY, MAX_SET_REPLY2 = USER_NAME_LEN + 23 + TOPIC_LEN + 1, 22 + TOPIC_LEN + 1, 17
#: their slots among a set call's texts (kSetHereRow .. kSetReply2Row), laid out as _ACCESS_ROWS lays an access call's
_SET_ROWS = (96, 84, 20)
_SET_COM_RULE = f"com must be one of the fourteen commands of SET_COMS {SET_COMS}"
#: the texts of an event in a Settings, in that order: the room line first, then the actor's two
SET_HERE, SET_REPLY, SET_REPLY2 = range(3)
#: the names of colcom[1 .. 20] (nuts333.c colcom, without ``RS`` at 0), and the twenty lines the video test of ``.colour``
#: writes, a ``write_user`` each (nuts333.c:7466-7469): what the caller sends for SET_COLOUR_TEST
_COLCOM = ("OL", "UL", "LI", "RV", "FK", "FR", "FG", "FY", "FB", "FM", "FT", "FW", "BK", "BR", "BG", "BY", "BB", "BM", "BT", "BW")
COLOUR_TEST = tuple(f"{c}: ~{c}NUTS 3 VIDEO TEST~RS\n".encode() for c in _COLCOM)
#: a look room's row of the names relay_many uploads (kRelayNameRow of fanout.hip): 20 bytes of name padded with zeros, then
#: its length; and what a relay text is longer than its broadcast at most, ``~FT[ `` + a 20-byte name + `` ]:~RS ``
#: (kRelaySlack): its slot among a relay call's relay texts is that much wider than the text
_RELAY_NAME_ROW, _RELAY_SLACK = 24, 32
#: the relay text's fixed bytes: ``~FT[ `` and `` ]:~RS ``
RELAY_EXTRA = 12


def max_bytes(text_len: int) -> int:
    """Hard bound on the bytes one item of ``text_len`` input bytes produces (a colour '\\n' is 6, plus the reset)."""
    return 6 * text_len + 4


@dataclass
class Fanout:
    admitted: np.ndarray          # bool [M]
    out_offsets: np.ndarray       # int64 [M + 1]
    arena: np.ndarray             # uint8 [out_offsets[-1]]
    write_offsets: np.ndarray     # int64 [M + 1]
    write_sizes: np.ndarray       # int32 [write_offsets[-1]]
    timing: dict = field(default_factory=dict)   # kernels_us (device events), end_to_end_us (host clock, H2D..D2H+sync)
    broadcast_offsets: np.ndarray | None = None  # broadcast_many: int64 [K + 1], broadcast k's items are [bo[k], bo[k+1])

    def output(self, i: int) -> bytes:
        return self.arena[self.out_offsets[i]:self.out_offsets[i + 1]].tobytes()

    def item(self, k: int, j: int) -> int:
        """The flat index of listener ``j`` of broadcast ``k`` in a :func:`broadcast_many` result."""
        if self.broadcast_offsets is None:
            raise ValueError("not a broadcast_many result: it has no broadcast_offsets")
        bo = self.broadcast_offsets
        if not 0 <= k < len(bo) - 1 or not 0 <= j < bo[k + 1] - bo[k]:
            raise IndexError(f"no item ({k}, {j}): {len(bo) - 1} broadcasts, "
                             f"broadcast {k} has {int(bo[k + 1] - bo[k]) if 0 <= k < len(bo) - 1 else 0} listeners")
        return int(bo[k] + j)


def _split(data: bytes, sizes: np.ndarray, what: str, holder: str) -> list[bytes]:
    """``data`` cut into consecutive chunks of ``sizes`` bytes, which must use it up."""
    out, at = [], 0
    for s in sizes.tolist():
        out.append(data[at:at + s])
        at += s
    if at != len(data):
        raise AssertionError(f"{what}: chunk sizes sum to {at}, {holder} holds {len(data)} bytes")
    return out


def chunks(result: Fanout, i: int) -> list[bytes]:
    """Item ``i`` as the list of ``write(2)`` chunks the reference would issue."""
    sizes = result.write_sizes[result.write_offsets[i]:result.write_offsets[i + 1]]
    return _split(result.output(i), sizes, f"item {i}", "arena slot")


def _offsets(counts, dtype, total: bool = False) -> np.ndarray:
    """Where each piece starts when pieces of ``counts`` elements lie one after another; with ``total`` one entry more,
    where they end."""
    off = np.zeros(len(counts) + 1, dtype=dtype)
    np.cumsum(counts, out=off[1:])
    return off if total else off[:-1]


def _gather(src: np.ndarray, starts: np.ndarray, counts: np.ndarray, step: int = 1 << 24) -> np.ndarray:
    """``concatenate([src[s:s + n] for s, n in zip(starts, counts)])`` without a Python loop over the pieces: index
    arithmetic over runs of pieces of about ``step`` elements, so that the index arrays stay small."""
    ends = np.cumsum(counts)
    total = int(ends[-1]) if len(ends) else 0
    out = np.empty(total, dtype=src.dtype)
    lo, at = 0, 0
    while lo < len(counts):
        hi = max(int(np.searchsorted(ends, at + step, side="right")), lo + 1)
        n = int(ends[hi - 1]) - at
        first = ends[lo:hi] - counts[lo:hi] - at          # where each piece starts in this run's output
        out[at:at + n] = src[np.repeat(starts[lo:hi] - first, counts[lo:hi]) + np.arange(n, dtype=np.int64)]
        lo, at = hi, at + n
    return out


def _variant_at(text_off, t):
    """Where text ``t``, whose bytes start at ``text_off`` among the call's texts, has its two variants in the variant
    buffer (var_at of fanout.hip); ``_variant_at(text bytes, texts)`` is the buffer's size."""
    return 12 * text_off + 16 * t


def _variant_starts(text_starts: np.ndarray, sizes: np.ndarray) -> np.ndarray:
    """int64 [..., 2]: the two variant slots of every text, the texts numbered in the arrays' own order; the second slot
    follows the first's hard bound, max_bytes(size) rounded up to 4 (var_stride of fanout.hip; a text that is not
    there, size -1, counts as empty)."""
    starts = np.empty(text_starts.shape + (2,), dtype=np.int64)
    t = np.arange(text_starts.size, dtype=np.int64).reshape(text_starts.shape)
    starts[..., 0] = _variant_at(text_starts.astype(np.int64), t)
    starts[..., 1] = starts[..., 0] + ((max_bytes(np.maximum(sizes, 0).astype(np.int64)) + 3) & ~3)
    return starts


def _composed_at(text_off, t, slack=_SPEAK_SLACK):
    """Where composed text ``t``, whose inpstr starts at ``text_off`` among the call's, has its slot in a speech call's
    text buffer (ctext_at of fanout.hip): room line k is text k, its reply text K + k over the same inpstr once more.
    ``_composed_at(2 * text bytes, 2 * K)`` is the buffer's size.  A private speech call's slots are ``_TELL_SLACK``
    wider than inpstr (ptext_at)."""
    return text_off + slack * t


def _unpack(words: np.ndarray, capacity: int) -> np.ndarray:
    """uint64 [..., W] bitmap words -> bool [..., capacity]: bit j % 64 of word j // 64 is slot j."""
    b = np.ascontiguousarray(words, dtype="<u8").view(np.uint8)
    return np.unpackbits(b, axis=-1, bitorder="little")[..., :capacity].astype(bool)


def _pack(flags: np.ndarray) -> np.ndarray:
    """bool [capacity] -> uint64 [W] bitmap words, the tail bits of the last word zero."""
    padded = np.zeros((len(flags) + 63) // 64 * 64, dtype=bool)
    padded[:len(flags)] = flags
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


class _Variants:
    """Two variants (colour off, colour on) per entry in one flat buffer, with their ``write(2)`` chunk sizes: the
    fields ``variants``, ``variant_starts``, ``variant_sizes``, ``write_counts`` and ``write_sizes`` that a
    :class:`Plan` and a :class:`Review` share.  ``_what`` names an entry in their messages."""

    def variant(self, k: int, c: int) -> bytes:
        """The bytes entry ``k`` sends to a listener with colour bit ``c``."""
        self._check(k, c)
        at = int(self.variant_starts[k, c])
        return self.variants[at:at + int(self.variant_sizes[k, c])].tobytes()

    def chunks(self, k: int, c: int) -> list[bytes]:
        """``variant(k, c)`` as the list of ``write(2)`` chunks the reference would issue."""
        return _split(self.variant(k, c), self.write_sizes[k, c, :int(self.write_counts[k, c])],
                      f"{self._what} ({k}, {c})", "the variant")


@dataclass
class Plan(_Variants):
    """What a talker needs to deliver K broadcasts to a roster: slot ``j`` gets ``variant(k, colour of j)``, in the
    chunks ``chunks(k, colour of j)``, if it is admitted.  :meth:`expand` replicates that into a :class:`Fanout`."""
    capacity: int
    admitted_bits: np.ndarray     # uint64 [K, W]  bit j % 64 of word j // 64 is slot j; bits past capacity are zero
    colour_bits: np.ndarray       # uint64 [W]     the roster's colour flags when the call was made (a copy)
    variants: np.ndarray          # uint8, flat; gaps between variants are allowed and unspecified
    variant_starts: np.ndarray    # int64 [K, 2]   variant c of broadcast k is variants[start : start + size]
    variant_sizes: np.ndarray     # int64 [K, 2]
    write_counts: np.ndarray      # int32 [K, 2]
    write_sizes: np.ndarray       # int32 [K, 2, MAX_WRITES]; entries at or past write_counts are unspecified
    timing: dict = field(default_factory=dict)   # as Roster.broadcast_many's: kernels_us, end_to_end_us, h2d/d2h_bytes
    _what = "variant"

    def _check(self, k: int, c=0) -> None:
        if not 0 <= k < len(self.admitted_bits) or c not in (0, 1):
            raise IndexError(f"no variant ({k}, {c}): {len(self.admitted_bits)} broadcasts, colour 0 or 1")

    def admitted(self, k: int) -> np.ndarray:
        """bool [capacity]: the slots broadcast ``k`` is delivered to."""
        self._check(k)
        return _unpack(self.admitted_bits[k], self.capacity)

    def recipients(self, k: int, c: int) -> np.ndarray:
        """The admitted slots of broadcast ``k`` whose colour bit is ``c``, ascending."""
        self._check(k, c)
        return np.flatnonzero(self.admitted(k) & (_unpack(self.colour_bits, self.capacity) == bool(c)))

    def expand(self) -> Fanout:
        """The :class:`Fanout` that ``Roster.broadcast_many`` returns for the same call (``timing`` aside), from this
        plan's own arrays alone: item ``(k, j)`` is ``variant(k, colour of j)`` if slot ``j`` is admitted."""
        k, cap = len(self.admitted_bits), self.capacity
        admitted = _unpack(self.admitted_bits, cap).reshape(k * cap)
        colour = _unpack(self.colour_bits, cap).astype(np.intp)
        sizes = np.asarray(self.variant_sizes, dtype=np.int64)[:, colour].reshape(k * cap)
        writes = np.asarray(self.write_counts, dtype=np.int64)[:, colour].reshape(k * cap)
        out_off = _offsets(np.where(admitted, sizes, 0), np.int64, total=True)
        w_off = _offsets(np.where(admitted, writes, 0), np.int64, total=True)
        items = np.flatnonzero(admitted)
        var = 2 * (items // cap) + colour[items % cap]                    # each admitted item's variant, as 2k + c
        arena = _gather(np.asarray(self.variants, dtype=np.uint8),
                        np.asarray(self.variant_starts, dtype=np.int64).reshape(2 * k)[var], sizes[items])
        wsz = _gather(np.asarray(self.write_sizes, dtype=np.int32).reshape(2 * k * MAX_WRITES), var * MAX_WRITES,
                      writes[items])
        return Fanout(admitted=admitted, out_offsets=out_off, arena=arena, write_offsets=w_off, write_sizes=wsz,
                      timing=dict(self.timing), broadcast_offsets=np.arange(k + 1, dtype=np.int64) * cap)


@dataclass
class Review(_Variants):
    """What ``.review`` sends for each of Q rooms, between its header and its footer: with ``line_0 ..`` the non-empty
    lines of the room's ring from the cursor onwards, ``chunks(q, c) == chunks(line_0, c) + chunks(line_1, c) + ...``
    (one ``write_user`` per line, so with colour on every line ends in a 4-byte reset write of its own) and
    ``variant(q, c) == b"".join(chunks(q, c))``."""
    rooms: np.ndarray             # int32 [Q]      the rooms asked for, duplicates included (revtell_many: the slots)
    line_counts: np.ndarray       # int32 [Q]      non-empty lines
    stored: np.ndarray            # uint8 [Q, 15, 202]  the ring's slots, oldest first; a line ends at its first NUL
    #                               (revtell_many: [Q, 5, 202], and MAX_REVTELL_WRITES chunk sizes per variant)
    variants: np.ndarray          # uint8, flat; gaps between variants are allowed and unspecified
    variant_starts: np.ndarray    # int64 [Q, 2]   variant c of room q is variants[start : start + size]
    variant_sizes: np.ndarray     # int64 [Q, 2]
    write_counts: np.ndarray      # int32 [Q, 2]
    write_sizes: np.ndarray       # int32 [Q, 2, MAX_REVIEW_WRITES]; entries at or past write_counts are unspecified
    sequential: np.ndarray | None = None         # int32 [Q] (line, variant) pairs the device transduced sequentially
    timing: dict = field(default_factory=dict)   # kernels_us, end_to_end_us, h2d_bytes, d2h_bytes
    _what = "review"

    def _check(self, q: int, c=0) -> None:
        if not 0 <= q < len(self.rooms) or c not in (0, 1):
            raise IndexError(f"no review ({q}, {c}): {len(self.rooms)} rooms, colour 0 or 1")

    def lines(self, q: int) -> list[bytes]:
        """The non-empty lines stored in room ``q``'s ring, as stored, oldest first."""
        self._check(q)
        out = [bytes(row).split(b"\0", 1)[0] for row in np.asarray(self.stored[q], dtype=np.uint8)]
        return [line for line in out if line]


@dataclass
class Speech:
    """What ``say()``, ``shout()``, ``emote()`` and ``semote()`` write for K speech events (``Roster.speak_many``).
    ``outcome[k]`` is SPOKEN, MUZZLED, NOTHING or SWEARING.  ``room`` plans the line the room (or every room) gets, K
    entries: ``room.admitted(k)`` is empty and both variants are 0 bytes in 0 writes when event ``k`` was not spoken.
    ``reply`` plans what the speaker alone gets -- the echo of a say or a shout, or the notice: ``reply.admitted(k)`` is
    the speaker's slot alone when there is a reply, else empty with zero sizes (a spoken emote or semote has none: no
    ``write_user`` call at all, which is not the 4-byte reset of an empty text).  Both are ordinary plans and share one
    variant buffer.  ``line(k)`` / ``reply_text(k)`` are the composed texts before the transducer.  In the ``Speech`` of
    an :class:`Input` the outcome of a read that no speech command answers is NOT_SPEECH: it has neither text, but for
    the reply ``Unknown command.`` of an UNKNOWN read."""
    outcome: np.ndarray           # int8 [K]
    room: Plan
    reply: Plan
    texts: np.ndarray             # uint8, flat: the composed texts; gaps are allowed and unspecified
    text_starts: np.ndarray       # int64 [2, K]   row 0 the room lines, row 1 the replies
    text_sizes: np.ndarray        # int64 [2, K]   -1: there is no such text
    timing: dict = field(default_factory=dict)   # as Plan's: kernels_us, end_to_end_us, h2d_bytes, d2h_bytes

    def _text(self, row: int, k: int) -> bytes:
        if not 0 <= k < len(self.outcome):
            raise IndexError(f"no event {k}: {len(self.outcome)} events")
        at, n = int(self.text_starts[row, k]), int(self.text_sizes[row, k])
        return self.texts[at:at + n].tobytes() if n >= 0 else b""

    def line(self, k: int) -> bytes:
        """The line event ``k`` sends to its room, or to every room; ``b""`` when it was not spoken (a composed line
        is never empty: it ends in a newline)."""
        return self._text(0, k)

    def reply_text(self, k: int) -> bytes:
        """What event ``k`` sends to its speaker alone: the echo or the notice; ``b""`` when there is none."""
        return self._text(1, k)


@dataclass
class Private:
    """What ``tell()`` and ``pemote()`` write for K private speech events (``Roster.tell_many``), shaped like a
    :class:`Speech`.  ``outcome[k]`` is TOLD, MUZZLED, NOTHING, NOBODY, SELF, AFK, IGNALL, IGNTELL or OFFSITE;
    ``target[k]`` the slot ``get_user`` found, or -1 when nobody was found or the lookup was never reached (MUZZLED,
    NOTHING, a pemote to one's own exact name).  ``told`` plans the line the target gets: ``told.admitted(k)`` is the
    target's slot alone for a TOLD event, else empty with both variants 0 bytes in 0 writes.  ``reply`` plans what the
    speaker alone gets, the echo or the notice; it always has a text.  Both are ordinary plans and share one variant
    buffer.  ``line(k)`` / ``reply_text(k)`` are the composed texts before the transducer."""
    outcome: np.ndarray           # int8 [K]
    target: np.ndarray            # int32 [K]
    told: Plan
    reply: Plan
    texts: np.ndarray             # uint8, flat: the composed texts; gaps are allowed and unspecified
    text_starts: np.ndarray       # int64 [2, K]   row 0 the told lines, row 1 the replies
    text_sizes: np.ndarray        # int64 [2, K]   -1: there is no such text
    timing: dict = field(default_factory=dict)   # as Plan's: kernels_us, end_to_end_us, h2d_bytes, d2h_bytes

    _text = Speech._text

    def line(self, k: int) -> bytes:
        """The line event ``k`` sends to its target; ``b""`` when it was not told."""
        return self._text(0, k)

    def reply_text(self, k: int) -> bytes:
        """What event ``k`` sends to its speaker alone: the echo or the notice."""
        return self._text(1, k)


@dataclass
class Look:
    """What ``look()`` writes for K lookers (``Roster.look_many``), as a delivery plan: texts with two variants each, and
    per looker which of them it gets.  The texts, T = 5 R + 3 + L of them for the R distinct rooms and L lines of the call:
    text ``5 i + j`` is text ``j`` (LOOK_NAME, LOOK_DESC, LOOK_EXITS, LOOK_ACCESS, LOOK_TOPIC) of room ``rooms[i]``;
    texts ``5 R``, ``5 R + 1`` and ``5 R + 2`` are ``You can see:``, ``You are all alone here.`` and the newline after the
    list; text ``5 R + 3 + l`` is line ``l``, the line of slot ``line_slots[l]``, transduced once however many lookers
    list it.  ``variants`` .. ``write_sizes`` hold their two variants as a :class:`Plan` holds a broadcast's, ``texts`` ..
    ``text_sizes`` the composed texts before the transducer (size -1: no such text).  Looker ``k`` is slot ``slots[k]``
    with colour bit ``colour[k]`` in room ``rooms[room_index[k]]``; its members are ``member_slots[member_starts[k]:][:
    member_counts[k]]`` in slot order and their lines ``member_lines`` alike.  ``timing`` is as a Plan's."""
    slots: np.ndarray             # int32 [K]
    colour: np.ndarray            # uint8 [K]   the lookers' colour bits
    room_index: np.ndarray        # int32 [K]   into rooms
    rooms: np.ndarray             # int32 [R]   the distinct rooms, in the order of their first looker
    member_slots: np.ndarray      # int32, flat
    member_lines: np.ndarray      # int32, flat: line numbers
    member_starts: np.ndarray     # int64 [K]
    member_counts: np.ndarray     # int32 [K]
    line_slots: np.ndarray        # int32 [L]   -1: a line nobody took
    texts: np.ndarray             # uint8, flat: the composed texts; gaps are allowed and unspecified
    text_starts: np.ndarray       # int64 [T]
    text_sizes: np.ndarray        # int64 [T]   -1: there is no such text
    variants: np.ndarray          # uint8, flat
    variant_starts: np.ndarray    # int64 [T, 2]
    variant_sizes: np.ndarray     # int64 [T, 2]
    write_counts: np.ndarray      # int32 [T, 2]
    write_sizes: np.ndarray       # int32 [T, 2, MAX_WRITES]   entries at or past write_counts are unspecified
    timing: dict = field(default_factory=dict)

    def _check(self, k: int) -> None:
        if not 0 <= k < len(self.slots):
            raise IndexError(f"no look {k}: {len(self.slots)} looks")

    def members(self, k: int) -> np.ndarray:
        """The slots look ``k`` lists, in list order."""
        self._check(k)
        at = int(self.member_starts[k])
        return self.member_slots[at:at + int(self.member_counts[k])]

    def text_numbers(self, k: int) -> list[int]:
        """The texts look ``k`` is sent, in look()'s order: one ``write_user`` each."""
        self._check(k)
        i, fixed = 5 * int(self.room_index[k]), 5 * len(self.rooms)
        at, n = int(self.member_starts[k]), int(self.member_counts[k])
        listed = [fixed] + [fixed + 3 + int(l) for l in self.member_lines[at:at + n]] if n else [fixed + 1]
        return [i + LOOK_NAME, i + LOOK_DESC, i + LOOK_EXITS] + listed + [fixed + 2, i + LOOK_ACCESS, i + LOOK_TOPIC]

    def text(self, t: int) -> bytes:
        """Text ``t`` before the transducer."""
        if not 0 <= t < len(self.text_sizes) or self.text_sizes[t] < 0:
            raise IndexError(f"no text {t}")
        at = int(self.text_starts[t])
        return self.texts[at:at + int(self.text_sizes[t])].tobytes()

    def text_chunks(self, t: int, c: int) -> list[bytes]:
        """Text ``t`` for colour bit ``c`` as the ``write(2)`` chunks the reference would issue."""
        if not 0 <= t < len(self.text_sizes) or c not in (0, 1):
            raise IndexError(f"no text ({t}, {c})")
        at = int(self.variant_starts[t, c])
        return _split(self.variants[at:at + int(self.variant_sizes[t, c])].tobytes(),
                      self.write_sizes[t, c, :int(self.write_counts[t, c])], f"text ({t}, {c})", "the variant")

    def chunks(self, k: int) -> list[bytes]:
        """The ``write(2)`` payloads of look ``k``, in order."""
        c = int(self.colour[k]) if 0 <= k < len(self.slots) else 0
        return [ch for t in self.text_numbers(k) for ch in self.text_chunks(t, c)]

    def output(self, k: int) -> bytes:
        """Everything look ``k`` writes: the concatenation of ``chunks(k)``."""
        return b"".join(self.chunks(k))


@dataclass
class Who:
    """What ``who(user, 0)`` writes for K lookers (``Roster.who_many``), as a delivery plan like a :class:`Look`: texts
    with two variants each, and per looker which of them it gets.  The texts, T = 4 + L of them for the L listed users:
    WHO_HEAD_LOGIN (the header of a looker at the name prompt), WHO_HEAD, WHO_FOOT and WHO_TAIL, then text ``4 + l`` is
    line ``l``, the line of slot ``line_slots[l]``, transduced once however many lookers are sent it.  ``texts`` ..
    ``write_sizes`` are exactly as in a Look.  Looker ``k`` is slot ``slots[k]`` with colour bit ``colour[k]`` and login
    flag ``login[k]``; it is sent line ``l`` iff bit ``l % 32`` of ``shown[k, l // 32]`` is set (bits at or past L are
    zero): a bitmap like a :class:`Plan`'s, since K x L flat lists would dominate the download."""
    slots: np.ndarray             # int32 [K]
    colour: np.ndarray            # uint8 [K]   the lookers' colour bits
    login: np.ndarray             # uint8 [K]   and whether they are at the name prompt
    line_slots: np.ndarray        # int32 [L]
    shown: np.ndarray             # uint32 [K, max(1, ceil(L / 32))]
    texts: np.ndarray             # uint8, flat: the composed texts; gaps are allowed and unspecified
    text_starts: np.ndarray       # int64 [T]
    text_sizes: np.ndarray        # int64 [T]
    variants: np.ndarray          # uint8, flat
    variant_starts: np.ndarray    # int64 [T, 2]
    variant_sizes: np.ndarray     # int64 [T, 2]
    write_counts: np.ndarray      # int32 [T, 2]
    write_sizes: np.ndarray       # int32 [T, 2, MAX_WRITES]   entries at or past write_counts are unspecified
    timing: dict = field(default_factory=dict)

    def _check(self, k: int) -> None:
        if not 0 <= k < len(self.slots):
            raise IndexError(f"no who {k}: {len(self.slots)} whos")

    def lines(self, k: int) -> np.ndarray:
        """The lines who ``k`` is sent, ascending."""
        self._check(k)
        bits = np.unpackbits(np.ascontiguousarray(self.shown[k], dtype="<u4").view(np.uint8), bitorder="little")
        return np.flatnonzero(bits[:len(self.line_slots)])

    def text_numbers(self, k: int) -> list[int]:
        """The texts who ``k`` is sent, in who()'s order: one ``write_user`` each."""
        listed = [4 + int(l) for l in self.lines(k)]
        return [WHO_HEAD_LOGIN if self.login[k] else WHO_HEAD] + listed + [WHO_FOOT, WHO_TAIL]

    def text(self, t: int) -> bytes:
        """Text ``t`` before the transducer."""
        if not 0 <= t < len(self.text_sizes) or self.text_sizes[t] < 0:
            raise IndexError(f"no text {t}")
        at = int(self.text_starts[t])
        return self.texts[at:at + int(self.text_sizes[t])].tobytes()

    def text_chunks(self, t: int, c: int) -> list[bytes]:
        """Text ``t`` for colour bit ``c`` as the ``write(2)`` chunks the reference would issue."""
        if not 0 <= t < len(self.text_sizes) or c not in (0, 1):
            raise IndexError(f"no text ({t}, {c})")
        at = int(self.variant_starts[t, c])
        return _split(self.variants[at:at + int(self.variant_sizes[t, c])].tobytes(),
                      self.write_sizes[t, c, :int(self.write_counts[t, c])], f"text ({t}, {c})", "the variant")

    def chunks(self, k: int) -> list[bytes]:
        """The ``write(2)`` payloads of who ``k``, in order."""
        self._check(k)
        c = int(self.colour[k])
        return [ch for t in self.text_numbers(k) for ch in self.text_chunks(t, c)]

    def output(self, k: int) -> bytes:
        """Everything who ``k`` writes: the concatenation of ``chunks(k)``."""
        return b"".join(self.chunks(k))


@dataclass
class Rooms:
    """What ``rooms(user, show_topics)`` writes for K lookers (``Roster.rooms_many``), as a delivery plan like a
    :class:`Who`: texts with two variants each, and per looker which of them it gets.  The texts, T = 3 + 2 R of them for
    the R look rooms: ROOMS_HEAD_TOPICS, ROOMS_HEAD_LINKS and ROOMS_TAIL, then text ``3 + r`` is room r's ``.rmst`` line
    and text ``3 + R + r`` its ``.rmsn`` line.  A room without a name is not listed: its lines have size -1.  So have the
    header and the lines of a kind that no looker of the call asks for, and they have no variants.  ``texts`` ..
    ``write_sizes`` are exactly as in a Look.  Looker ``k`` is slot ``slots[k]`` with colour bit ``colour[k]``; it typed
    ``.rmst`` when ``topics[k]`` is set, else ``.rmsn``, and is sent that kind's header, that kind's line of every listed
    room in ascending room number, and the tail.  ``counts[r]`` is the number of users the device counted in room r."""
    slots: np.ndarray             # int32 [K]
    colour: np.ndarray            # uint8 [K]   the lookers' colour bits
    topics: np.ndarray            # uint8 [K]   1: .rmst, 0: .rmsn
    counts: np.ndarray            # int32 [R]
    texts: np.ndarray             # uint8, flat: the composed texts; gaps are allowed and unspecified
    text_starts: np.ndarray       # int64 [T]
    text_sizes: np.ndarray        # int64 [T]   -1: there is no such text
    variants: np.ndarray          # uint8, flat
    variant_starts: np.ndarray    # int64 [T, 2]
    variant_sizes: np.ndarray     # int64 [T, 2]
    write_counts: np.ndarray      # int32 [T, 2]
    write_sizes: np.ndarray       # int32 [T, 2, MAX_WRITES]   entries at or past write_counts are unspecified
    timing: dict = field(default_factory=dict)

    def text_numbers(self, k: int) -> list[int]:
        """The texts looker ``k`` is sent, in rooms()'s order: one ``write_user`` each."""
        if not 0 <= k < len(self.slots):
            raise IndexError(f"no rooms {k}: {len(self.slots)} lookers")
        nr = len(self.counts)
        first = 3 if self.topics[k] else 3 + nr
        listed = [first + r for r in range(nr) if self.text_sizes[first + r] >= 0]
        return [ROOMS_HEAD_TOPICS if self.topics[k] else ROOMS_HEAD_LINKS] + listed + [ROOMS_TAIL]

    text = Who.text
    text_chunks = Who.text_chunks

    def chunks(self, k: int) -> list[bytes]:
        """The ``write(2)`` payloads of looker ``k``, in order."""
        numbers = self.text_numbers(k)
        c = int(self.colour[k])
        return [ch for t in numbers for ch in self.text_chunks(t, c)]

    def output(self, k: int) -> bytes:
        """Everything looker ``k`` writes: the concatenation of ``chunks(k)``."""
        return b"".join(self.chunks(k))


@dataclass
class Relay:
    """What ``write_room_except`` does with K broadcasts for a roster with clone records (``Roster.relay_many``): ``plan``
    is the :class:`Plan` of the same broadcasts for the slots, and clone record ``c`` relays broadcast ``k`` iff bit
    ``c % 64`` of ``relay_bits[k, c // 64]`` is set.  The relay text of broadcast ``k`` is ``relay_text(k)``, with its
    two variants and their ``write(2)`` chunk sizes as a Plan holds a broadcast's; all of them are empty, 0 bytes in 0
    writes, when no record relays ``k``.  ``clone_owner`` and ``owner_colour`` are the records' owners (-1: an empty
    record) and the owners' colour bits when the call was made, from the host mirrors.

    Delivery: for broadcast ``k`` a talker writes ``plan.variant(k, colour of j)`` to every admitted slot ``j``, then, for
    every record ``c`` of ``relays(k)`` in ascending order, ``relay_variant(k, owner_colour[c])`` to ``clone_owner[c]``."""
    plan: Plan
    clones: int
    relay_bits: np.ndarray        # uint64 [K, CW]  CW = ceil(clones / 64); bits past the records are zero
    clone_owner: np.ndarray       # int32 [C]       a copy of the records' owners
    owner_colour: np.ndarray      # uint8 [C]       the owners' colour bits (0 for an empty record)
    texts: np.ndarray             # uint8, flat: the relay texts; gaps are allowed and unspecified
    text_starts: np.ndarray       # int64 [K]
    text_sizes: np.ndarray        # int64 [K]   -1: nothing relays
    variants: np.ndarray          # uint8, flat
    variant_starts: np.ndarray    # int64 [K, 2]
    variant_sizes: np.ndarray     # int64 [K, 2]
    write_counts: np.ndarray      # int32 [K, 2]
    write_sizes: np.ndarray       # int32 [K, 2, MAX_WRITES]; entries at or past write_counts are unspecified
    timing: dict = field(default_factory=dict)   # as Plan's: kernels_us, end_to_end_us, h2d_bytes, d2h_bytes

    def _check(self, k: int, c=0) -> None:
        if not 0 <= k < len(self.relay_bits) or c not in (0, 1):
            raise IndexError(f"no relay ({k}, {c}): {len(self.relay_bits)} broadcasts, colour 0 or 1")

    def relays(self, k: int) -> np.ndarray:
        """The clone records that relay broadcast ``k``, ascending."""
        self._check(k)
        return np.flatnonzero(_unpack(self.relay_bits[k], self.clones))

    def owners(self, k: int) -> np.ndarray:
        """The slots the relay of broadcast ``k`` is written to, one per record of ``relays(k)`` and in its order; an
        owner of two relaying records is there twice."""
        return self.clone_owner[self.relays(k)]

    def owner_colours(self, k: int) -> np.ndarray:
        """The colour bits of ``owners(k)``."""
        return self.owner_colour[self.relays(k)]

    def relay_text(self, k: int) -> bytes:
        """``b"~FT[ " + room name + b" ]:~RS " + text`` of broadcast ``k``; ``b""`` when nothing relays it."""
        self._check(k)
        at, n = int(self.text_starts[k]), int(self.text_sizes[k])
        return self.texts[at:at + n].tobytes() if n >= 0 else b""

    def relay_variant(self, k: int, c: int) -> bytes:
        """The bytes an owner with colour bit ``c`` gets of broadcast ``k``."""
        self._check(k, c)
        at = int(self.variant_starts[k, c])
        return self.variants[at:at + int(self.variant_sizes[k, c])].tobytes()

    def relay_chunks(self, k: int, c: int) -> list[bytes]:
        """``relay_variant(k, c)`` as the list of ``write(2)`` chunks the reference would issue."""
        return _split(self.relay_variant(k, c), self.write_sizes[k, c, :int(self.write_counts[k, c])],
                      f"relay ({k}, {c})", "the variant")


@dataclass
class Go:
    """What ``go()`` and ``move_user()`` write for K ``.go`` events (``Roster.go_many``), shaped like a :class:`Speech`.
    ``outcome[k]`` is GO_WALKED, GO_TELEPORTED or GO_UNSEEN for an event that moved, else GO_WHERE, GO_NETLINK, GO_NO_ROOM,
    GO_ALREADY, GO_NOT_ADJOINED, GO_PRIVATE or GO_DEFERRED; ``target[k]`` the room the word resolved to, or -1 when there is
    none or ``get_room`` was not reached; ``old_room[k]`` the mover's room before the call; ``returned_public[k]`` whether
    the move made the old room public again.  ``enter`` plans the line the target room gets, ``leave`` the line the old
    room gets without the mover, ``reset`` the line the old room gets when it returns to public, ``reply`` the notice the
    mover alone gets when it did not move.  They are ordinary plans over the roster as it was before the call and share
    one variant buffer; a text that is not there has size -1, nobody admitted and both variants 0 bytes in 0 writes.  A
    GO_NETLINK and a GO_DEFERRED event have no text at all, and a deferred event's ``target`` and ``old_room`` are what the
    roster before the call gives.  ``look`` is the :class:`Look` of the movers after the moves,
    in event order, or None when nobody moved, and ``look_index[k]`` event k's looker in it, or -1.

    Delivery, per client: the events in call order, and of one event the enter line, the leave line, the mover's look,
    the reset line (``reply`` instead of all four for an event that did not move).  A roster with clone records passes
    the three room texts through ``relay_many``."""
    outcome: np.ndarray           # int8 [K]
    target: np.ndarray            # int32 [K]
    old_room: np.ndarray          # int32 [K]
    returned_public: np.ndarray   # bool [K]
    enter: Plan
    leave: Plan
    reset: Plan
    reply: Plan
    texts: np.ndarray             # uint8, flat: the composed texts; gaps are allowed and unspecified
    text_starts: np.ndarray       # int64 [4, K]   rows GO_ENTER, GO_LEAVE, GO_RESET, GO_REPLY
    text_sizes: np.ndarray        # int64 [4, K]   -1: there is no such text
    look: Look | None = None
    look_index: np.ndarray | None = None         # int32 [K]
    timing: dict = field(default_factory=dict)   # the first device visit's, as Plan's; the second's is look.timing

    _text = Speech._text

    def enter_text(self, k: int) -> bytes:
        """The line event ``k`` sends to the room it enters; ``b""`` when it did not move."""
        return self._text(GO_ENTER, k)

    def leave_text(self, k: int) -> bytes:
        """The line event ``k`` sends to the room it leaves; ``b""`` when it did not move."""
        return self._text(GO_LEAVE, k)

    def reset_text(self, k: int) -> bytes:
        """The line the room event ``k`` left gets when it returns to public; ``b""`` when it does not."""
        return self._text(GO_RESET, k)

    def reply_text(self, k: int) -> bytes:
        """The notice event ``k`` sends to its mover alone; ``b""`` when there is none."""
        return self._text(GO_REPLY, k)

    def moved(self) -> np.ndarray:
        """The events that moved, ascending."""
        return np.flatnonzero((self.outcome >= 0) & (self.outcome <= GO_UNSEEN))


@dataclass
class Access:
    """What ``set_room_access()``, ``letmein()`` and ``invite()`` write for K events (``Roster.access_many``), shaped like a
    :class:`Go`.  ``outcome[k]`` is one of the ACCESS_* constants; ``target_room[k]`` the room the event is about -- the
    actor's own for a ``.public`` / ``.private`` without a word, else the room the word resolved to -- or -1 when
    ``get_room`` found none or was not reached (an ``.invite`` never asks it: its room is the actor's); ``target_slot[k]``
    the slot ``get_user`` found, or -1 when it found none or was not reached.  ``reply`` plans the actor's own line,
    ``here`` the line the actor's room gets without the actor, ``there`` the line another room gets, ``notice`` the line
    an invited user gets, whatever its ``ignall``, ``afk`` and room.  They are ordinary plans over the roster as it was
    before the call and share one variant buffer; a text that is not there has size -1, nobody admitted and both
    variants 0 bytes in 0 writes.  An ACCESS_DEFERRED event has no text at all, and its targets are what the roster
    before the call gives.

    Delivery, per client: the events in call order, and of one event the reply, the here or the there line, the notice
    (the reference's order of writes).  A roster with clone records passes the two room lines through ``relay_many``."""
    outcome: np.ndarray           # int8 [K]
    target_room: np.ndarray       # int32 [K]
    target_slot: np.ndarray       # int32 [K]
    reply: Plan
    here: Plan
    there: Plan
    notice: Plan
    texts: np.ndarray             # uint8, flat: the composed texts; gaps are allowed and unspecified
    text_starts: np.ndarray       # int64 [4, K]   rows ACCESS_HERE, ACCESS_THERE, ACCESS_REPLY, ACCESS_NOTICE
    text_sizes: np.ndarray        # int64 [4, K]   -1: there is no such text
    timing: dict = field(default_factory=dict)

    _text = Speech._text

    def reply_text(self, k: int) -> bytes:
        """The line event ``k`` sends to its actor; ``b""`` for a deferred event."""
        return self._text(ACCESS_REPLY, k)

    def here_text(self, k: int) -> bytes:
        """The line event ``k`` sends to its actor's room without the actor; ``b""`` when there is none."""
        return self._text(ACCESS_HERE, k)

    def there_text(self, k: int) -> bytes:
        """The line event ``k`` sends to another room; ``b""`` when there is none."""
        return self._text(ACCESS_THERE, k)

    def notice_text(self, k: int) -> bytes:
        """The line event ``k`` sends to the user it invited; ``b""`` when it invited nobody."""
        return self._text(ACCESS_NOTICE, k)

    def effective(self) -> np.ndarray:
        """The events that set an access or invited someone, ascending."""
        return np.flatnonzero((self.outcome >= 0) & (self.outcome <= ACCESS_INVITED))


@dataclass
class Clone:
    """What ``create_clone()``, ``destroy_clone()``, ``clone_say()`` and ``clone_hear()`` write for K events
    (``Roster.clone_many``), shaped like an :class:`Access`.  ``outcome[k]`` is CLONE_HEAR_NOTHING, CLONE_HEAR_SWEARS or
    CLONE_HEAR_ALL for a ``.chear`` that was obeyed -- the value it set -- or one of the other CLONE_* constants;
    ``target_room[k]`` the room the event is about -- the actor's own for a ``.clone`` or ``.destroy`` without a word, else
    the room the word resolved to -- or -1 when ``get_room`` found none or was not reached; ``target_slot[k]`` the slot
    ``get_user`` found for a ``.destroy`` with a name, the owner, or -1 when it found none or was not asked; ``reset[k]``
    whether the room a destroyed clone left returned to public.  ``record[k]`` is the clone record the event found -- the
    one destroyed, spoken through, set, or already there --, an index into the records as they were before the call, and -1
    where there is none, as for a created one; ``created[k]`` is the record a CLONE_CREATED event was given, an index into
    the records as the call leaves them, and -1 for every other event.

    ``reply`` plans the actor's own line, ``here`` the line the actor's room gets without the actor, ``there`` the line the
    clone's room gets (without the actor for a created clone, whole for a destroyed one), ``reset_plan`` the line a room
    that returns to public gets, ``notice`` the line the owner of a clone that another destroyed gets, and ``said`` the
    line a clone speaks to its room.  They are ordinary plans over the roster as it was before the call and share one
    variant buffer; a text that is not there has size -1, nobody admitted and both variants 0 bytes in 0 writes.  A
    CLONE_DEFERRED event has no text at all, and its targets are what the roster before the call gives.

    Delivery, per client: the events in call order, and of one event the reset line, the reply, the here line, the there
    line, the notice (``destroy_clone``'s order of writes; a created clone has no reset line and no notice), or the said
    line alone.  The four room lines pass through ``relay_many``, over the records as the call leaves them."""
    outcome: np.ndarray           # int8 [K]
    target_room: np.ndarray       # int32 [K]
    target_slot: np.ndarray       # int32 [K]
    record: np.ndarray            # int32 [K]
    created: np.ndarray           # int32 [K]
    reset: np.ndarray             # bool [K]
    reply: Plan
    here: Plan
    there: Plan
    reset_plan: Plan
    notice: Plan
    said: Plan
    texts: np.ndarray             # uint8, flat: the composed texts; gaps are allowed and unspecified
    text_starts: np.ndarray       # int64 [6, K]   rows CLONE_HERE, CLONE_THERE, CLONE_RESET, CLONE_SAID_LINE, CLONE_REPLY, CLONE_NOTICE
    text_sizes: np.ndarray        # int64 [6, K]   -1: there is no such text
    timing: dict = field(default_factory=dict)

    _text = Speech._text

    def reply_text(self, k: int) -> bytes:
        """The line event ``k`` sends to its actor; ``b""`` for a clone that spoke and for a deferred event."""
        return self._text(CLONE_REPLY, k)

    def here_text(self, k: int) -> bytes:
        """The line event ``k`` sends to its actor's room without the actor; ``b""`` when there is none."""
        return self._text(CLONE_HERE, k)

    def there_text(self, k: int) -> bytes:
        """The line event ``k`` sends to the clone's room; ``b""`` when there is none."""
        return self._text(CLONE_THERE, k)

    def reset_text(self, k: int) -> bytes:
        """The line event ``k`` sends to a room that returns to public; ``b""`` when none does."""
        return self._text(CLONE_RESET, k)

    def notice_text(self, k: int) -> bytes:
        """The line event ``k`` sends to the owner of the clone it destroyed; ``b""`` when that is the actor, or nobody."""
        return self._text(CLONE_NOTICE, k)

    def said_text(self, k: int) -> bytes:
        """The line the clone of event ``k`` speaks; ``b""`` when none spoke."""
        return self._text(CLONE_SAID_LINE, k)

    def effective(self) -> np.ndarray:
        """The events that set a ``clone_hear``, created a clone, destroyed one or made one speak, ascending."""
        return np.flatnonzero((self.outcome >= 0) & (self.outcome <= CLONE_SAID))


@dataclass
class Act:
    """What ``move()``, ``wake()``, ``muzzle()`` and ``unmuzzle()`` write for K events (``Roster.act_many``), shaped like a
    :class:`Clone`.  ``outcome[k]`` is one of the ACT_* constants; ``target_slot[k]`` the slot ``get_user`` found, or -1 when
    it found none or was not asked; ``target_room[k]`` the room the event is about -- the room ``word[2]`` of a ``.move``
    resolved to, the actor's own without such a word -- or -1 when ``get_room`` found none or was not reached;
    ``old_room[k]`` the found slot's room before the call, the room a move leaves, or -1 without a slot;
    ``returned_public[k]`` whether the move made that room public again.

    ``reply`` plans the actor's own line, ``here`` the chant line the actor's room gets without the actor, ``enter`` the
    line the room entered gets, ``leave`` the line the room left gets without the target, ``reset`` the line a room that
    returns to public gets, and ``notice`` the target's own line: the giant hand (a visible target only), the wake-up
    call, or the word of a muzzle set or removed.  They are ordinary plans over the roster as it was before the call and
    share one variant buffer; a text that is not there has size -1, nobody admitted and both variants 0 bytes in 0 writes.
    ACT_MOVE_AWAY, the two ``*_ABSENT`` outcomes, ACT_UNMUZZLE_NOT and ACT_DEFERRED have no text at all, and a deferred
    event's targets are what the roster before the call gives.  ``look`` is the :class:`Look` of the moved targets after
    the moves, in event order, or None when nobody moved, and ``look_index[k]`` event k's looker in it, or -1.

    Delivery, per client: the events in call order, and of one event the reply, the here line, the notice, the enter line,
    the leave line, the target's look, the reset line.  A roster with clone records passes the four room lines through
    ``relay_many``."""
    outcome: np.ndarray           # int8 [K]
    target_slot: np.ndarray       # int32 [K]
    target_room: np.ndarray       # int32 [K]
    old_room: np.ndarray          # int32 [K]
    returned_public: np.ndarray   # bool [K]
    reply: Plan
    here: Plan
    enter: Plan
    leave: Plan
    reset: Plan
    notice: Plan
    texts: np.ndarray             # uint8, flat: the composed texts; gaps are allowed and unspecified
    text_starts: np.ndarray       # int64 [6, K]   rows ACT_HERE, ACT_ENTER, ACT_LEAVE, ACT_RESET, ACT_REPLY, ACT_NOTICE
    text_sizes: np.ndarray        # int64 [6, K]   -1: there is no such text
    look: Look | None = None
    look_index: np.ndarray | None = None         # int32 [K]
    timing: dict = field(default_factory=dict)   # the first device visit's, as Plan's; the second's is look.timing

    _text = Speech._text

    def reply_text(self, k: int) -> bytes:
        """The line event ``k`` sends to its actor; ``b""`` when there is none."""
        return self._text(ACT_REPLY, k)

    def here_text(self, k: int) -> bytes:
        """The chant line event ``k`` sends to its actor's room without the actor; ``b""`` when nobody moved."""
        return self._text(ACT_HERE, k)

    def enter_text(self, k: int) -> bytes:
        """The line event ``k`` sends to the room its target enters; ``b""`` when nobody moved."""
        return self._text(ACT_ENTER, k)

    def leave_text(self, k: int) -> bytes:
        """The line event ``k`` sends to the room its target leaves; ``b""`` when nobody moved."""
        return self._text(ACT_LEAVE, k)

    def reset_text(self, k: int) -> bytes:
        """The line the room event ``k``'s target left gets when it returns to public; ``b""`` when it does not."""
        return self._text(ACT_RESET, k)

    def notice_text(self, k: int) -> bytes:
        """The line event ``k`` sends to its target alone; ``b""`` when there is none."""
        return self._text(ACT_NOTICE, k)

    def moved(self) -> np.ndarray:
        """The events that moved their target, ascending."""
        return np.flatnonzero((self.outcome >= 0) & (self.outcome <= ACT_MOVED_UNSEEN))

    def effective(self) -> np.ndarray:
        """The events that moved a user, set a muzzle or removed one, ascending."""
        return np.flatnonzero((self.outcome >= 0) & (self.outcome <= ACT_UNMUZZLED))


@dataclass
class Settings:
    """What the commands a user sets its own state with write for K events (``Roster.set_many``), shaped like an
    :class:`Access`.  ``outcome[k]`` is one of the SET_* constants.  ``reply`` plans the actor's first ``write_user``,
    ``reply2`` its second -- only an ``.afk`` that set a message has one, ``"AFK message set.\\n"``, a ``write(2)`` of its own
    -- and ``here`` the line ``write_room_except(user->room, text, user)`` sends: the actor's room without the actor,
    without ``login`` slots and without ``ignall`` listeners.  They are ordinary plans over the roster as it was before the
    call and share one variant buffer; a text that is not there has size -1, nobody admitted and both variants 0 bytes in 0
    writes.  A SET_DEFERRED event has no text at all; SET_COLOUR_TEST has none either, its twenty lines are COLOUR_TEST.

    ``reply_colour[k]`` is the colour the actor's two replies are written with: the roster's flag, but 1 for SET_COLOUR_ON
    and SET_COLOUR_OFF, since the reference writes both while ``user->colour`` is 1 (it sets the flag before the write and
    clears it after, nuts333.c:7472-7479).  A ``.colour`` reply is therefore delivered by ``reply_colour``, not by
    ``reply.colour_bits``, which hold the flags before the call.

    Delivery, per client: the events in call order, and of one event ``reply``, ``reply2``, ``here`` (the reference's order
    of writes).  A roster with clone records passes the here lines through ``relay_many``; that of a SET_IGNALL_ON with
    ``ignall={actor: 0}`` and that of a SET_IGNALL_OFF with ``ignall={actor: 1}``, the flag as it was while the reference
    wrote the line (nuts333.c:4466-4476)."""
    outcome: np.ndarray           # int8 [K]
    reply: Plan
    reply2: Plan
    here: Plan
    reply_colour: np.ndarray      # uint8 [K]
    texts: np.ndarray             # uint8, flat: the composed texts; gaps are allowed and unspecified
    text_starts: np.ndarray       # int64 [3, K]   rows SET_HERE, SET_REPLY, SET_REPLY2
    text_sizes: np.ndarray        # int64 [3, K]   -1: there is no such text
    timing: dict = field(default_factory=dict)

    _text = Speech._text

    def reply_text(self, k: int) -> bytes:
        """The first line event ``k`` sends to its actor; ``b""`` for a deferred event and for the video test."""
        return self._text(SET_REPLY, k)

    def reply2_text(self, k: int) -> bytes:
        """The second line event ``k`` sends to its actor; ``b""`` when there is none."""
        return self._text(SET_REPLY2, k)

    def here_text(self, k: int) -> bytes:
        """The line event ``k`` sends to its actor's room without the actor; ``b""`` when there is none."""
        return self._text(SET_HERE, k)

    def effective(self) -> np.ndarray:
        """The events that changed something, ascending."""
        return np.flatnonzero((self.outcome >= 0) & (self.outcome <= SET_IGNTELL_OFF))


@dataclass
class Input:
    """What ``user_input()`` and ``exec_com()`` make of K reads (``Roster.input_many``).  ``kind[k]`` is IAC, EMPTY,
    REPEAT, UNKNOWN, SPEECH or COMMAND; ``com[k]`` the command (enum np_com) of a SPEECH or COMMAND read, else -1;
    ``word_count[k]`` the talker's, 0 .. 9 (0 for IAC); the line is ``data[:line_sizes[k]]`` (0 for IAC, which is not
    framed) and ``inpstr(k)`` what the command function receives, for a SPEECH or COMMAND read.  ``speech`` has K
    entries: a SPEECH read's is what ``speak_many`` returns for ``(slot, com, inpstr, word_count)`` -- except a say
    that came through ``exec_com`` with fewer than two words, which is NOTHING (``Say what?``) whatever the speaker's
    muzzle and mode --, an UNKNOWN read's has the reply ``Unknown command.`` and no line, every other read's is void;
    the outcome of all that is not SPEECH is NOT_SPEECH."""
    kind: np.ndarray              # int8 [K]
    com: np.ndarray               # int8 [K]   -1: none
    word_count: np.ndarray        # uint8 [K]
    line_sizes: np.ndarray        # int32 [K]
    inpstr_starts: np.ndarray     # int64 [K]  into read k's own data
    inpstr_sizes: np.ndarray      # int64 [K]  -1: there is no inpstr
    speech: Speech
    data: list = field(default_factory=list)     # the K reads' bytes, as given
    timing: dict = field(default_factory=dict)   # as Speech's

    def inpstr(self, k: int) -> bytes:
        """What the command function of read ``k`` receives; ``b""`` when there is none."""
        if not 0 <= k < len(self.kind):
            raise IndexError(f"no read {k}: {len(self.kind)} reads")
        at, n = int(self.inpstr_starts[k]), int(self.inpstr_sizes[k])
        return bytes(self.data[k][at:at + n]) if n >= 0 else b""

    def line(self, k: int) -> bytes:
        """Read ``k`` cut at its first control byte."""
        if not 0 <= k < len(self.kind):
            raise IndexError(f"no read {k}: {len(self.kind)} reads")
        return bytes(self.data[k][:int(self.line_sizes[k])])


# ------------------------------------------------------------------ validation (never touches the device)
def _as_bytes(what: str, v) -> bytes:
    """bytes as they are, a str as latin-1, a bytearray or memoryview as a copy; ``what`` names the value."""
    if isinstance(v, str):
        try:
            v = v.encode("latin-1")
        except UnicodeEncodeError as e:
            raise ValueError(f"{what} has a character outside one byte: {e}") from None
    elif isinstance(v, (bytearray, memoryview)):
        v = bytes(v)
    if not isinstance(v, bytes):
        raise ValueError(f"{what} must be bytes or str, not {type(v).__name__}")
    return v


def _is_int(v, lo: int, hi: int) -> bool:
    """An int, numpy's included, that is not a bool and lies in [lo, hi]."""
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and lo <= int(v) <= hi


def _as_text(t) -> bytes:
    t = _as_bytes("text", t)
    if b"\0" in t:
        raise ValueError("text contains a NUL byte (the talker's strings end there)")
    if len(t) >= TEXT_SIZE:
        raise ValueError(f"text of {len(t)} bytes: the talker's text buffer holds at most {TEXT_SIZE - 1}")
    return t


def _remove_first(inpstr: bytes) -> bytes:
    """``remove_first()`` (nuts333.c:2350-2358): ``inpstr`` behind its first word and the blanks around it.  A word byte
    is above 32 as a signed char."""
    word = lambda c: 32 < c < 128
    pos, n = 0, len(inpstr)
    while pos < n and not word(inpstr[pos]):
        pos += 1
    while pos < n and word(inpstr[pos]):
        pos += 1
    while pos < n and not word(inpstr[pos]):
        pos += 1
    return inpstr[pos:]


def _flag(name: str, v) -> int:
    if isinstance(v, (bool, np.bool_)) or (isinstance(v, (int, np.integer)) and int(v) in (0, 1)):
        return int(v)
    raise ValueError(f"{name} must be 0/1 or a bool, not {v!r}")


def _listener_records(listeners) -> np.ndarray:
    """(N, 7) 0/1 table in LISTENER_FIELDS order -> one byte per listener (bit k = column k)."""
    try:
        a = np.asarray(listeners)
    except Exception as e:   # ragged nested lists
        raise ValueError(f"listeners are not a table: {e}") from None
    if a.ndim != 2 or a.shape[1] != len(LISTENER_FIELDS):
        raise ValueError(f"listeners must have shape (N, {len(LISTENER_FIELDS)}) with columns {LISTENER_FIELDS}, "
                         f"got {a.shape}")
    if a.shape[0] == 0:
        raise ValueError("empty broadcast: no listeners")
    if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"listener records must be integers or bools, got {a.dtype}")
    if not np.isin(a, (0, 1)).all():
        raise ValueError("listener record fields must be 0 or 1")
    bits = (a.astype(np.uint8) << np.arange(len(LISTENER_FIELDS), dtype=np.uint8)).sum(axis=1)
    return np.ascontiguousarray(bits.astype(np.uint8))


def _prepare_batch(texts, colours):
    texts = [_as_text(t) for t in texts]
    if not texts:
        raise ValueError("empty batch")
    colours = list(colours)
    if len(colours) != len(texts):
        raise ValueError(f"{len(texts)} texts but {len(colours)} colour bits")
    rec = np.array([_flag("colour", c) for c in colours], dtype=np.uint8) << 6
    lens = np.fromiter((len(t) for t in texts), dtype=np.int32, count=len(texts))
    if int(lens.sum(dtype=np.int64)) >= 2**31:
        raise ValueError("batch text larger than 2 GiB: split it")
    return b"".join(texts), _offsets(lens, np.int32), lens, rec


def _prepare_broadcast(text, listeners, rm_is_null, force_listen, com_num):
    text = _as_text(text)
    rec = _listener_records(listeners)
    flags = _flag("rm_is_null", rm_is_null), _flag("force_listen", force_listen)
    return text, rec, flags[0], flags[1], _com_num(com_num)


def _com_num(v) -> int:
    if not _is_int(v, 0, NUM_COMMANDS - 1):
        raise ValueError(f"com_num must be a command number in [0, {NUM_COMMANDS}), not {v!r}")
    return int(v)


def _prepare_many(broadcasts):
    """Each (text, listeners, rm_is_null, force_listen, com_num) through _prepare_broadcast, packed for
    nd_fanout_many: texts, text offsets and lengths, flags (bit 0 rm_is_null, bit 1 force_listen), commands, item
    offsets [K + 1] and the listener records, one byte each."""
    if isinstance(broadcasts, (str, bytes, bytearray, np.ndarray)) or not hasattr(broadcasts, "__len__"):
        raise ValueError(f"broadcasts must be a sequence of tuples, not {type(broadcasts).__name__}")
    if len(broadcasts) == 0:
        raise ValueError("empty call: no broadcasts")
    texts, recs, flags, coms = [], [], [], []
    for k, b in enumerate(broadcasts):
        if not isinstance(b, tuple) or len(b) != 5:
            raise ValueError(f"broadcast {k}: expected a (text, listeners, rm_is_null, force_listen, com_num) tuple, "
                             f"got {type(b).__name__}{f' of {len(b)}' if isinstance(b, tuple) else ''}")
        try:
            text, rec, rm_is_null, force_listen, com_num = _prepare_broadcast(*b)
        except ValueError as e:
            raise ValueError(f"broadcast {k}: {e}") from None
        texts.append(text)
        recs.append(rec)
        flags.append(rm_is_null | force_listen << 1)
        coms.append(com_num)
    lens = np.fromiter((len(t) for t in texts), dtype=np.int64, count=len(texts))
    ns = np.fromiter((len(r) for r in recs), dtype=np.int64, count=len(recs))
    bound = int((ns * (6 * lens + 4)).sum())
    if bound > MANY_ARENA_CAP:
        raise ValueError(f"call too large: its arena bound is {bound} bytes, the cap is {MANY_ARENA_CAP} "
                         f"(MANY_ARENA_CAP): split it")
    return (b"".join(texts), _offsets(lens, np.int32), lens.astype(np.int32), np.array(flags, dtype=np.uint8),
            np.array(coms, dtype=np.int32), _offsets(ns, np.int32, total=True), np.concatenate(recs))


# ------------------------------------------------------------------ the library
class _Timing(ctypes.Structure):
    _fields_ = [("kernels_us", ctypes.c_double), ("end_to_end_us", ctypes.c_double)]


class _RosterTiming(ctypes.Structure):
    _fields_ = [("kernels_us", ctypes.c_double), ("end_to_end_us", ctypes.c_double),
                ("h2d_bytes", ctypes.c_int64), ("d2h_bytes", ctypes.c_int64)]


_LIB = None


def hipcc() -> str | None:
    return shutil.which("hipcc") or next((p for p in ("/opt/rocm/bin/hipcc",) if os.access(p, os.X_OK)), None)


def build_library(force: bool = False, timeout: float = 600) -> Path:
    """Compile fanout.hip for gfx950 into _build/libnuts_device.so (when missing, stale, or ``force``)."""
    if not force and LIBRARY.exists() and LIBRARY.stat().st_mtime >= SOURCE.stat().st_mtime:
        return LIBRARY
    cc = hipcc()
    if cc is None:
        raise RuntimeError("hipcc not found: cannot build nuts333_amd/device/_build/libnuts_device.so")
    LIBRARY.parent.mkdir(exist_ok=True)
    tmp = LIBRARY.with_name(f".{LIBRARY.name}.{os.getpid()}")
    subprocess.run([cc, "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", str(SOURCE), "-o", str(tmp)],
                   check=True, timeout=timeout)
    os.replace(tmp, LIBRARY)
    return LIBRARY


def _load():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(str(build_library()))
        lib.nd_last_error.restype = ctypes.c_char_p
        lib.nd_device_count.restype = ctypes.c_int
        P = ctypes.c_void_p
        lib.nd_fanout.argtypes = [ctypes.c_int, P, ctypes.c_int64, P, P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_int, P, P, P, ctypes.POINTER(_Timing)]
        lib.nd_fanout.restype = ctypes.c_int
        lib.nd_fanout_many.argtypes = [ctypes.c_int, P, ctypes.c_int64, P, P, P, P, P, P, P, P, P,
                                       ctypes.POINTER(_Timing)]
        lib.nd_fanout_many.restype = ctypes.c_int
        lib.nd_roster_create.argtypes = [ctypes.c_int]
        lib.nd_roster_create.restype = ctypes.c_int
        lib.nd_roster_destroy.argtypes = [ctypes.c_int]
        lib.nd_roster_destroy.restype = ctypes.c_int
        lib.nd_roster_fanout.argtypes = [ctypes.c_int, ctypes.c_int, P, ctypes.c_int64, P, P, P, P, P, P, P, P, P, P,
                                         ctypes.POINTER(_RosterTiming)]
        lib.nd_roster_fanout.restype = ctypes.c_int
        lib.nd_roster_plan.argtypes = [ctypes.c_int, ctypes.c_int, P, ctypes.c_int64, P, P, P, P, P, P, P, P, P, P, P,
                                       P, ctypes.POINTER(_RosterTiming)]
        lib.nd_roster_plan.restype = ctypes.c_int
        lib.nd_roster_plan_record.argtypes = lib.nd_roster_plan.argtypes + [P]
        lib.nd_roster_plan_record.restype = ctypes.c_int
        lib.nd_roster_review_rooms.argtypes = [ctypes.c_int, ctypes.c_int]
        lib.nd_roster_review_rooms.restype = ctypes.c_int
        lib.nd_roster_review.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, P, P, P, P, P, P,
                                         ctypes.POINTER(_RosterTiming)]
        lib.nd_roster_review.restype = ctypes.c_int
        lib.nd_roster_speak.argtypes = [ctypes.c_int, ctypes.c_int, P, ctypes.c_int64, P, P, P, P, P, ctypes.c_int,
                                        ctypes.c_int, P, P, P, P, P, P, P, P, P, P, P, ctypes.POINTER(_RosterTiming)]
        lib.nd_roster_speak.restype = ctypes.c_int
        lib.nd_roster_input.argtypes = [ctypes.c_int, ctypes.c_int, P, ctypes.c_int64, P, P, P, ctypes.c_int,
                                        ctypes.c_int, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P,
                                        ctypes.POINTER(_RosterTiming)]
        lib.nd_roster_input.restype = ctypes.c_int
        lib.nd_roster_revtell_rings.argtypes = [ctypes.c_int]
        lib.nd_roster_revtell_rings.restype = ctypes.c_int
        lib.nd_roster_revtell.argtypes = lib.nd_roster_review.argtypes
        lib.nd_roster_revtell.restype = ctypes.c_int
        lib.nd_roster_tell.argtypes = [ctypes.c_int, ctypes.c_int, P, ctypes.c_int64, P, P, P, P, P, ctypes.c_int,
                                       P, P, P, P, P, P, P, P, P, P, P, P, ctypes.POINTER(_RosterTiming)]
        lib.nd_roster_tell.restype = ctypes.c_int
        lib.nd_roster_look_rooms.argtypes = [ctypes.c_int, ctypes.c_int]
        lib.nd_roster_look_rooms.restype = ctypes.c_int
        lib.nd_roster_look.argtypes = [ctypes.c_int, ctypes.c_int, P, P, ctypes.c_int] + [P] * 18 + [ctypes.POINTER(_RosterTiming)]
        lib.nd_roster_look.restype = ctypes.c_int
        lib.nd_roster_who.argtypes = ([ctypes.c_int, ctypes.c_int, P, ctypes.c_int, ctypes.c_int32, P, ctypes.c_int] + [P] * 13
                                      + [ctypes.POINTER(_RosterTiming)])
        lib.nd_roster_who.restype = ctypes.c_int
        lib.nd_roster_rooms.argtypes = [ctypes.c_int, ctypes.c_int, P, ctypes.c_int] + [P] * 10 + [ctypes.POINTER(_RosterTiming)]
        lib.nd_roster_rooms.restype = ctypes.c_int
        lib.nd_roster_go.argtypes = ([ctypes.c_int, ctypes.c_int, P, ctypes.c_int64, P, P, P, P, ctypes.c_int, ctypes.c_int] + [P] * 16
                                     + [ctypes.POINTER(_RosterTiming)])
        lib.nd_roster_go.restype = ctypes.c_int
        lib.nd_roster_access.argtypes = ([ctypes.c_int, ctypes.c_int, P, ctypes.c_int64, P, P, P, P, P, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int] + [P] * 15 + [ctypes.POINTER(_RosterTiming)])
        lib.nd_roster_access.restype = ctypes.c_int
        lib.nd_roster_clone.argtypes = ([ctypes.c_int, ctypes.c_int, P, ctypes.c_int64, P, P, P, P, P, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int] + [P] * 18 + [ctypes.POINTER(_RosterTiming)])
        lib.nd_roster_clone.restype = ctypes.c_int
        lib.nd_roster_act.argtypes = ([ctypes.c_int, ctypes.c_int, P, ctypes.c_int64, P, P, P, P, P, ctypes.c_int, ctypes.c_int]
                                      + [P] * 17 + [ctypes.POINTER(_RosterTiming)])
        lib.nd_roster_act.restype = ctypes.c_int
        lib.nd_roster_set.argtypes = [ctypes.c_int, ctypes.c_int, P, ctypes.c_int64] + [P] * 19 + [ctypes.POINTER(_RosterTiming)]
        lib.nd_roster_set.restype = ctypes.c_int
        lib.nd_roster_clones.argtypes = [ctypes.c_int, ctypes.c_int]
        lib.nd_roster_clones.restype = ctypes.c_int
        lib.nd_roster_relay.argtypes = [ctypes.c_int, ctypes.c_int, P, ctypes.c_int64] + [P] * 22 + [ctypes.POINTER(_RosterTiming)]
        lib.nd_roster_relay.restype = ctypes.c_int
        lib.nd_roster_relay_record.argtypes = lib.nd_roster_relay.argtypes + [P]
        lib.nd_roster_relay_record.restype = ctypes.c_int
        lib.nd_arena.restype = P
        lib.nd_write_sizes.restype = P
        _LIB = lib
    return _LIB


def _check(rc: int, what: str) -> int:
    """What a call of the library returned, or ``RuntimeError("what: the library's message")`` when it is negative."""
    if rc < 0:
        raise RuntimeError(f"{what}: {_LIB.nd_last_error().decode(errors='replace')}")
    return rc


def _timing_of(t) -> dict:
    """A call's timing struct as the dict its result carries: kernels_us and end_to_end_us, and a roster call's
    h2d_bytes and d2h_bytes."""
    return {name: getattr(t, name) for name, _ in t._fields_}


def device_count() -> int:
    """Visible GPUs (loads, and if needed builds, the library; does not allocate on the device)."""
    n = _load().nd_device_count()
    if n < 0:
        raise RuntimeError(_LIB.nd_last_error().decode(errors="replace"))
    return n


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def _run(broadcast: bool, text: bytes, offs, lens, rec, rm_is_null=0, force_listen=0, com_num=0) -> Fanout:
    lib = _load()
    n = len(rec)
    admitted = np.zeros(n, dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.int64)
    w_off = np.zeros(n + 1, dtype=np.int32)
    tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
    t = _Timing()
    rc = lib.nd_fanout(int(broadcast), _ptr(tbuf), len(text), _ptr(offs) if offs is not None else None, _ptr(lens),
                       _ptr(rec), n, rm_is_null, force_listen, com_num, _ptr(admitted), _ptr(out_off), _ptr(w_off),
                       ctypes.byref(t))
    _check(rc, "device fan-out failed")
    return _result(lib, admitted, out_off, w_off, t)


def _result(lib, admitted, out_off, w_off, t) -> Fanout:
    """The Fanout of the last call: the arena and the chunk sizes copied out of the library's pinned buffers."""
    nbytes, nwrites = int(out_off[-1]), int(w_off[-1])
    arena = np.ctypeslib.as_array(ctypes.cast(lib.nd_arena(), ctypes.POINTER(ctypes.c_uint8)), (max(nbytes, 1),))
    wsz = np.ctypeslib.as_array(ctypes.cast(lib.nd_write_sizes(), ctypes.POINTER(ctypes.c_int32)), (max(nwrites, 1),))
    return Fanout(admitted=admitted.astype(bool), out_offsets=out_off, arena=arena[:nbytes].copy(),
                  write_offsets=w_off.astype(np.int64), write_sizes=wsz[:nwrites].copy(),
                  timing=_timing_of(t))


def transduce_batch(texts, colours) -> Fanout:
    """M independent (text, colour) items through the transducer; every item is admitted."""
    text, offs, lens, rec = _prepare_batch(texts, colours)
    return _run(False, text, offs, lens, rec)


def broadcast(text, listeners, rm_is_null, force_listen, com_num) -> Fanout:
    """One text to N listeners.  ``listeners``: (N, 7) table of 0/1 in LISTENER_FIELDS order."""
    text, rec, rm_is_null, force_listen, com_num = _prepare_broadcast(text, listeners, rm_is_null, force_listen, com_num)
    lens = np.array([len(text)], dtype=np.int32)
    return _run(True, text, None, lens, rec, rm_is_null, force_listen, com_num)


def broadcast_many(broadcasts) -> Fanout:
    """K broadcasts in one device call: a sequence of ``(text, listeners, rm_is_null, force_listen, com_num)`` tuples,
    each what :func:`broadcast` takes and checked by the same rules.  Items are ordered broadcast by broadcast, listeners
    in table order; ``broadcast_offsets[k]:broadcast_offsets[k + 1]`` are broadcast k's (``Fanout.item(k, j)``).  A call
    whose arena bound exceeds MANY_ARENA_CAP is refused (``ValueError``) before the device is touched."""
    text, text_off, lens, flags, coms, item_off, rec = _prepare_many(broadcasts)
    lib = _load()
    m = len(rec)
    admitted = np.zeros(m, dtype=np.uint8)
    out_off = np.zeros(m + 1, dtype=np.int64)
    w_off = np.zeros(m + 1, dtype=np.int32)
    tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
    t = _Timing()
    rc = lib.nd_fanout_many(len(lens), _ptr(tbuf), len(text), _ptr(text_off), _ptr(lens), _ptr(flags), _ptr(coms),
                            _ptr(item_off), _ptr(rec), _ptr(admitted), _ptr(out_off), _ptr(w_off), ctypes.byref(t))
    _check(rc, "device fan-out failed")
    r = _result(lib, admitted, out_off, w_off, t)
    r.broadcast_offsets = item_off.astype(np.int64)
    return r


# ------------------------------------------------------------------ a resident roster
#: a Roster's flag fields, stored as their listener-record bits (bit k = LISTENER_FIELDS[k])
ROSTER_FLAGS = {f: 1 << LISTENER_FIELDS.index(f) for f in ("login", "ignall", "ignshout", "colour")}
_KEEP = object()


def _room(v) -> int:
    """A room id: None (no room) is -1, else an int in [0, ROOM_LIMIT)."""
    if v is None:
        return -1
    if not _is_int(v, 0, ROOM_LIMIT - 1):
        raise ValueError(f"room must be None or an int in [0, {ROOM_LIMIT}), not {v!r}")
    return int(v)


def _speaker_name(v) -> bytes:
    """``user->name``: bytes or str of 1 .. USER_NAME_LEN bytes, no NUL."""
    v = _as_bytes("name", v)
    if not 1 <= len(v) <= USER_NAME_LEN or b"\0" in v:
        raise ValueError(f"name must be 1 .. {USER_NAME_LEN} bytes without a NUL, not {v!r}")
    return v


def _level(v) -> int:
    if not _is_int(v, 0, MAX_LEVEL):
        raise ValueError(f"level must be an int in [0, {MAX_LEVEL}] (enum np_level), not {v!r}")
    return int(v)


def _read_data(v) -> bytes:
    """One read(2) of a client in line mode: 1 .. READ_SIZE bytes of any value, the last one ending the line."""
    v = _as_bytes("data", v)
    if not 1 <= len(v) <= READ_SIZE:
        raise ValueError(f"data of {len(v)} bytes: a read holds 1 .. {READ_SIZE}")
    if 32 <= v[-1] < 128:
        raise ValueError(f"the read does not end a line (its last byte is {v[-1]}, not below 32 as a signed char): it "
                         f"belongs to get_charclient_line, whose per-user buffer the roster does not keep")
    return v


def _afk_mesg(v) -> bytes:
    """``user->afk_mesg``: bytes or str of 0 .. AFK_MESG_LEN bytes, no NUL."""
    v = _as_bytes("afk_mesg", v)
    if len(v) > AFK_MESG_LEN or b"\0" in v:
        raise ValueError(f"afk_mesg must be 0 .. {AFK_MESG_LEN} bytes without a NUL, not {v!r}")
    return v


def _limited_text(what: str, v, most: int) -> bytes:
    """A talker string of at most ``most`` bytes: bytes or str, one byte per character, no NUL."""
    v = _as_bytes(what, v)
    if len(v) > most or b"\0" in v:
        raise ValueError(f"{what} must be 0 .. {most} bytes without a NUL, not {v!r}")
    return v


def _one_or_each(what: str, v, n: int, conv, scalar) -> list:
    """``v`` as one converted value per entry: itself n times when ``scalar(v)``, else a sequence of n."""
    if scalar(v):
        return [conv(v)] * n
    if isinstance(v, (str, bytes, bytearray, memoryview)) or not hasattr(v, "__len__"):
        raise ValueError(f"{what} must be a value or a sequence of one per entry, not {v!r}")
    if len(v) != n:
        raise ValueError(f"{what}: {len(v)} values for {n} entries")
    return [conv(x) for x in v]


_is_text = lambda v: isinstance(v, (str, bytes, bytearray, memoryview))
_is_number = lambda v: isinstance(v, (int, np.integer, bool, np.bool_))


#: the commands speak_many answers, and whether their room line goes to the speaker's room (and is recorded there)
_SPEECH_COMS = {COM_SAY: True, COM_SHOUT: False, COM_EMOTE: True, COM_SEMOTE: False}


class Roster:
    """The talker's user list, kept on the device between calls: per slot a room (``None``: an empty slot, or a user
    away over a netlink) and the ``login``, ``ignall``, ``ignshout`` and ``colour`` flags.  Broadcasts are addressed as
    ``write_room_except(rm, str, user)`` addresses them (nuts333.c:1401-1415): ``rm`` is a room or ``None`` for every
    room, ``sender`` a slot or ``None``.  The device builds each listener's record from its slot and the broadcast, so a
    call carries K texts and K small tuples; the table travels only in the first call after an :meth:`update`.
    :meth:`broadcast_many` returns every slot's bytes in an arena (a :class:`Fanout`), :meth:`plan_many` the two variants
    and an admit bitmap per broadcast (a :class:`Plan`); they may be mixed in any order.  With ``review_rooms=R`` rooms
    ``0 .. R - 1`` each own a review ring on the device, empty at first: ``plan_many(bs, record=...)`` records into them,
    :meth:`review_many` reads them, :meth:`clear_review` empties them.  ``review_rooms=0`` is a roster without rings.
    With ``revtell=True`` every slot also owns a revtell ring on the device, 5 lines of 202 bytes and a cursor, empty at
    first (1,010 bytes per slot in an allocation of its own, 66 MB at MAX_CAPACITY, so it has to be asked for):
    ``tell_many(events, record=True)`` records into them, :meth:`revtell_many` reads them, :meth:`clear_revtell` empties
    them.
    With ``clones=C`` the roster also has clone records ``0 .. C - 1``, empty at first and kept apart from the slots
    (:meth:`set_clones`): a clone is not a slot, and only :meth:`relay_many` sees it.

    Building and updating a roster does not touch the device; its first call allocates there.  The
    contract, for every call::

        roster.broadcast_many(bs) == broadcast_many([(t, roster.table(rm, s), rm is None, fl, com)
                                                     for t, rm, s, fl, com in bs])
    """

    def __init__(self, capacity: int, review_rooms: int = 0, revtell: bool = False, look_rooms: int = 0, clones: int = 0):
        if not _is_int(capacity, 1, MAX_CAPACITY):
            raise ValueError(f"roster capacity must be an int in [1, {MAX_CAPACITY}], not {capacity!r}")
        if not _is_int(review_rooms, 0, MAX_REVIEW_ROOMS):
            raise ValueError(f"review_rooms must be an int in [0, {MAX_REVIEW_ROOMS}], not {review_rooms!r}")
        if not isinstance(revtell, (bool, np.bool_)):
            raise ValueError(f"revtell must be a bool, not {revtell!r}")
        if not _is_int(look_rooms, 0, MAX_LOOK_ROOMS):
            raise ValueError(f"look_rooms must be an int in [0, {MAX_LOOK_ROOMS}], not {look_rooms!r}")
        if not _is_int(clones, 0, MAX_CAPACITY):
            raise ValueError(f"clones must be an int in [0, {MAX_CAPACITY}], not {clones!r}")
        self.capacity = int(capacity)
        self.review_rooms = int(review_rooms)
        self.revtell = bool(revtell)
        # slots whose revtell ring clear_revtell() emptied since the last recording tell_many or revtell_many call
        self._tell_clear = np.zeros(self.capacity if self.revtell else 0, dtype=np.uint8)
        self._tell_clear_pending = False
        # rooms whose ring clear_review() emptied since the last recording or reviewing call: one byte per ring room
        self._clear = np.zeros(self.review_rooms, dtype=np.uint8)
        self._clear_pending = False
        # the host mirror, as nd_roster_fanout takes it: `capacity` int32 rooms (-1: none), then `capacity` flag bytes
        self._table = np.zeros(5 * self.capacity, dtype=np.uint8)
        self._room = self._table[:4 * self.capacity].view(np.int32)
        self._flags = self._table[4 * self.capacity:]
        self._room[:] = -1
        self._dirty = True
        # the speakers' mirror, as nd_roster_speak takes it: 16 bytes per slot -- 12 name bytes, the name's length, a
        # flags byte (SPEECH_FLAGS), the level, a byte of padding.  Only speak_many and input_many upload it, after an
        # update of its fields
        self._speech = np.zeros((self.capacity, 16), dtype=np.uint8)
        self._speech[:, USER_NAME_LEN + 1] = SPEECH_FLAGS["vis"]
        self._speech_dirty = True
        # afk and igntell live in the speaker mirror's flags byte, but only tell_many reads them: an update of theirs
        # alone makes tell_many upload the speaker mirror, and no other call
        self._private_dirty = False
        # prompt and charmode_echo live in that byte too, and only set_many reads them: an update of theirs alone makes
        # set_many upload the speaker mirror, and no other call
        self._set_dirty = False
        # the AFK messages' mirror, as nd_roster_tell takes it: 64 bytes per slot -- the message padded with zeros, then
        # its length at byte AFK_MESG_LEN.  Only tell_many uploads it, after an update of afk_mesg
        self._afk = np.zeros((self.capacity, _AFK_ROW), dtype=np.uint8)
        self._afk_dirty = True
        # what look_many alone reads and uploads: the room table -- a 256-byte record per look room, then an 816-byte
        # description row per look room (the fields are listed in fanout.hip's look section) -- after set_rooms, and the
        # users' descriptions, 32 bytes per slot -- 30 of description padded with zeros, then its length -- after
        # update(desc=)
        self.look_rooms = int(look_rooms)
        self._rooms = np.zeros(self.look_rooms * (_ROOM_REC + _ROOM_DESC_ROW), dtype=np.uint8)
        self._room_rec = self._rooms[:self.look_rooms * _ROOM_REC].reshape(self.look_rooms, _ROOM_REC)
        self._room_desc = self._rooms[self.look_rooms * _ROOM_REC:].reshape(self.look_rooms, _ROOM_DESC_ROW)
        self._rooms_dirty = True
        self._udesc = np.zeros((self.capacity, _DESC_ROW), dtype=np.uint8)
        self._udesc_dirty = True
        # what who_many alone reads and uploads beside those: 8 bytes per slot -- int32 last_login, int32 away (-1: none) --
        # after update(last_login=, away=)
        self._who = np.zeros((self.capacity, 2), dtype=np.int32)
        self._who[:, 1] = -1
        self._who_dirty = True
        # what relay_many alone reads and uploads: the clone records, kept apart from the slots -- `clones` int32 owners
        # (-1: an empty record), then `clones` int32 rooms, then `clones` clone_hear bytes -- after set_clones; and the look
        # rooms' names, 24 bytes per room, when one differs from those relay_many uploaded last (None: none yet)
        self.clones = int(clones)
        self._clones = np.zeros(9 * self.clones, dtype=np.uint8)
        self._clone_owner = self._clones[:4 * self.clones].view(np.int32)
        self._clone_room = self._clones[4 * self.clones:8 * self.clones].view(np.int32)
        self._clone_hear = self._clones[8 * self.clones:]
        self._clone_owner[:] = -1
        self._clone_room[:] = -1
        self._clones_dirty = True
        self._relay_names = None
        # what go_many alone reads and uploads: 88 bytes per slot -- in_phrase and its length, out_phrase and its length, int32
        # invite_room (-1: none) -- after update(in_phrase=, out_phrase=, invite_room=)
        self._go = np.zeros((self.capacity, _GO_REC), dtype=np.uint8)
        self._go_invite = self._go[:, _GO_INVITE:_GO_INVITE + 4].view(np.int32).reshape(self.capacity)
        self._go[:, :6], self._go[:, PHRASE_LEN] = np.frombuffer(b"enters", dtype=np.uint8), 6
        self._go[:, _GO_OUT:_GO_OUT + 4], self._go[:, _GO_OUT + PHRASE_LEN] = np.frombuffer(b"goes", dtype=np.uint8), 4
        self._go_invite[:] = -1
        self._go_dirty = True
        self._handle = None
        self._closed = False

    def _ring_rooms_are(self) -> str:
        return (f"the ring rooms are 0 .. {self.review_rooms - 1}" if self.review_rooms else
                "the roster has none (review_rooms is 0)")

    def _check_speaker(self, slot: int, recorded: str | None) -> None:
        """What a speech event or a read needs of its speaker: a room, no ``login`` flag, a name, and a ring room when
        ``recorded`` says why ("it is to be recorded", "it may be recorded"; None: it is not)."""
        if self._room[slot] < 0:
            raise ValueError(f"the speaker, slot {slot}, has no room (the talker relays such a user over its netlink)")
        if self._flags[slot] & ROSTER_FLAGS["login"]:
            raise ValueError(f"the speaker, slot {slot}, is still logging in")
        if self._speech[slot, USER_NAME_LEN] == 0:
            raise ValueError(f"the speaker, slot {slot}, has no name")
        if recorded and not 0 <= self._room[slot] < self.review_rooms:
            raise ValueError(f"{recorded}, but room {int(self._room[slot])} has no review ring: "
                             f"{self._ring_rooms_are()}")

    def _check_open(self) -> None:
        if self._closed:
            raise ValueError("the roster is closed")

    def _slot(self, v) -> int:
        if not _is_int(v, 0, self.capacity - 1):
            raise ValueError(f"slot must be an int in [0, {self.capacity}), not {v!r}")
        return int(v)

    def update(self, slots, *, room=_KEEP, login=_KEEP, ignall=_KEEP, ignshout=_KEEP, colour=_KEEP, name=_KEEP,
               vis=_KEEP, muzzled=_KEEP, command_mode=_KEEP, level=_KEEP, afk=_KEEP, igntell=_KEEP,
               afk_mesg=_KEEP, desc=_KEEP, last_login=_KEEP, away=_KEEP, in_phrase=_KEEP, out_phrase=_KEEP,
               invite_room=_KEEP, prompt=_KEEP, charmode_echo=_KEEP, muzzle_level=_KEEP) -> None:
        """Set fields of ``slots`` (a slot or a sequence of them).  Each field given is one value for every slot or a
        sequence of one per slot; a field not given stays as it is.  ``room`` is None (no room) or an int in
        [0, ROOM_LIMIT); the flags are 0/1 or bools.  A slot given more than once takes its last values.  Nothing
        changes unless the whole update is valid.

        ``name`` (bytes or str of 1 .. USER_NAME_LEN bytes, no NUL; unset at first), ``vis`` (1 at first), ``muzzled``
        and ``command_mode`` (0 at first) are what the speech commands read of a speaker.  They live in a mirror of
        their own that only :meth:`speak_many` uploads: an update of these fields alone does not make the next
        ``broadcast_many`` / ``plan_many`` upload the table.  ``level`` (an int in [0, MAX_LEVEL] as enum np_level, 0
        -- NEW -- at first) lives there too: :meth:`input_many` checks a command's minimum level against it, and
        ``speak_many`` does not read it.

        ``afk`` and ``igntell`` (0/1, 0 at first) and ``afk_mesg`` (bytes or str of 0 .. AFK_MESG_LEN bytes, no NUL,
        empty at first) are what :meth:`tell_many` reads of a **target**: a read that comes from an AFK slot remains
        the caller's business.  The two flags live in the speaker mirror's flags byte, with a dirty flag of their
        own; the messages in a mirror of their own.  Only ``tell_many`` uploads after an update of these three alone,
        and :meth:`act_many`, whose ``.wake`` reads a target's ``afk``, after one of the two flags: no other call copies
        more for it.

        ``desc`` (bytes or str of 0 .. USER_DESC_LEN bytes, no NUL, empty at first) is ``user->desc``, which ``look()``
        shows beside a name.  It lives in a mirror of its own that only :meth:`look_many` and :meth:`who_many` upload.

        ``last_login`` (an int in [0, 2^31), 0 at first) is ``user->last_login``, and ``away`` (None at first, or a look
        room whose record has a netlink) the link a user without a room left through, whose service ``who()`` shows in
        place of a room.  They live in a mirror of their own, 8 bytes per slot, that only ``who_many`` uploads: an update
        of these two alone marks no other mirror.

        ``in_phrase`` and ``out_phrase`` (bytes or str of 0 .. PHRASE_LEN bytes, no NUL; ``enters`` and ``goes`` at first, as
        a new user's are, nuts333.c:1575-1576) are what a walking user's room lines say, and ``invite_room`` (None at first,
        or a look room) the private room a user may enter by invitation.  They live in a mirror of their own, 88 bytes per
        slot, that only :meth:`go_many` uploads: an update of these three alone marks no other mirror.

        ``prompt`` and ``charmode_echo`` (0/1, 0 at first) are ``user->prompt`` and ``user->charmode_echo``, which
        ``.prompt``, ``.charecho`` and the video test of ``.colour`` read.  They live in the last two bits of the speaker
        mirror's flags byte, with a dirty flag of their own: only :meth:`set_many` uploads after an update of these two
        alone.

        ``muzzle_level`` (an int in [0, MAX_LEVEL], 0 at first) is ``user->muzzled``, the level of the user who set the
        muzzle.  It lives in byte 15 of a slot's speaker row, and setting it also sets the ``muzzled`` bit to ``level >
        0``; it marks the speaker mirror as ``level`` does.  ``muzzled`` stays what it was: it writes the bit and never
        byte 15, so the two cannot be given in one update.  :meth:`act_many` reads a slot's muzzle as byte 15 when the bit
        is set and the byte is not 0, as WIZ -- the lowest level that can type ``.muzzle`` -- when the bit is set over a
        byte of 0, and as 0 when the bit is clear; every other call reads the bit alone."""
        self._check_open()
        if isinstance(slots, (int, np.integer)):
            slots = [slots]
        try:
            idx = np.array([self._slot(s) for s in slots], dtype=np.int64)
        except TypeError:
            raise ValueError(f"slots must be a slot or a sequence of them, not {slots!r}") from None
        n = len(idx)

        def per_slot(name, v, conv, dtype):
            if v is None or isinstance(v, (int, np.integer, bool, np.bool_)):
                return np.full(n, conv(v), dtype=dtype)
            if isinstance(v, (str, bytes)) or not hasattr(v, "__len__"):
                raise ValueError(f"{name} must be a value or a sequence of one per slot, not {v!r}")
            if len(v) != n:
                raise ValueError(f"{name}: {len(v)} values for {n} slots")
            return np.array([conv(x) for x in v], dtype=dtype)

        rooms = None if room is _KEEP else per_slot("room", room, _room, np.int32)
        flags = {f: per_slot(f, v, lambda x, f=f: _flag(f, x), np.uint8)
                 for f, v in (("login", login), ("ignall", ignall), ("ignshout", ignshout), ("colour", colour))
                 if v is not _KEEP}
        names = None
        if name is not _KEEP:
            if isinstance(name, (str, bytes, bytearray, memoryview)):
                names = [_speaker_name(name)] * n
            elif not hasattr(name, "__len__"):
                raise ValueError(f"name must be a name or a sequence of one per slot, not {name!r}")
            elif len(name) != n:
                raise ValueError(f"name: {len(name)} values for {n} slots")
            else:
                names = [_speaker_name(x) for x in name]
        speech = {f: per_slot(f, v, lambda x, f=f: _flag(f, x), np.uint8)
                  for f, v in (("vis", vis), ("muzzled", muzzled), ("command_mode", command_mode), ("afk", afk),
                               ("igntell", igntell), ("prompt", prompt), ("charmode_echo", charmode_echo)) if v is not _KEEP}
        levels = None if level is _KEEP else per_slot("level", level, _level, np.uint8)
        if muzzle_level is not _KEEP and muzzled is not _KEEP:
            raise ValueError("muzzled and muzzle_level cannot be given in one update: muzzle_level sets the muzzled bit too")

        def muzzle(v):
            if not _is_int(v, 0, MAX_LEVEL):
                raise ValueError(f"muzzle_level must be an int in [0, {MAX_LEVEL}] (enum np_level), not {v!r}")
            return int(v)

        muzzles = None if muzzle_level is _KEEP else per_slot("muzzle_level", muzzle_level, muzzle, np.uint8)
        mesgs = None
        if afk_mesg is not _KEEP:
            if isinstance(afk_mesg, (str, bytes, bytearray, memoryview)):
                mesgs = [_afk_mesg(afk_mesg)] * n
            elif not hasattr(afk_mesg, "__len__"):
                raise ValueError(f"afk_mesg must be a message or a sequence of one per slot, not {afk_mesg!r}")
            elif len(afk_mesg) != n:
                raise ValueError(f"afk_mesg: {len(afk_mesg)} values for {n} slots")
            else:
                mesgs = [_afk_mesg(x) for x in afk_mesg]
        descs = None
        if desc is not _KEEP:
            descs = _one_or_each("desc", desc, n, lambda x: _limited_text("desc", x, USER_DESC_LEN), _is_text)
        def login_time(v):
            if not _is_int(v, 0, 2**31 - 1):
                raise ValueError(f"last_login must be an int in [0, 2^31), not {v!r}")
            return int(v)

        def away_room(v):
            if v is None:
                return -1
            if isinstance(v, (bool, np.bool_)):
                raise ValueError(f"away must be None or a look room, not {v!r}")
            v = self._look_room(v)
            if not self._room_rec[v, 24] & 1:
                raise ValueError(f"away: room {v} has no netlink")
            return v

        def invited(v):
            if v is None:
                return -1
            if isinstance(v, (bool, np.bool_)):
                raise ValueError(f"invite_room must be None or a look room, not {v!r}")
            return self._look_room(v)

        phrases = {f: _one_or_each(f, v, n, lambda x, f=f: _limited_text(f, x, PHRASE_LEN), _is_text)
                   for f, v in (("in_phrase", in_phrase), ("out_phrase", out_phrase)) if v is not _KEEP}
        invites = None if invite_room is _KEEP else per_slot("invite_room", invite_room, invited, np.int32)
        logins = None if last_login is _KEEP else per_slot("last_login", last_login, login_time, np.int32)
        aways = None if away is _KEEP else per_slot("away", away, away_room, np.int32)
        _, last = np.unique(idx[::-1], return_index=True)        # each slot's last position: last write wins
        keep = n - 1 - last
        at = idx[keep]
        if rooms is not None:
            self._room[at] = rooms[keep]
        for f, v in flags.items():
            bit = np.uint8(ROSTER_FLAGS[f])
            self._flags[at] = np.where(v[keep] != 0, self._flags[at] | bit, self._flags[at] & ~bit)
        if names is not None:
            for j, p in zip(at.tolist(), keep.tolist()):
                self._speech[j, :USER_NAME_LEN] = 0
                self._speech[j, :len(names[p])] = np.frombuffer(names[p], dtype=np.uint8)
                self._speech[j, USER_NAME_LEN] = len(names[p])
        for f, v in speech.items():
            bit, col = np.uint8(SPEECH_FLAGS.get(f) or SET_FLAGS[f]), self._speech[:, USER_NAME_LEN + 1]
            col[at] = np.where(v[keep] != 0, col[at] | bit, col[at] & ~bit)
        if levels is not None:
            self._speech[at, _LEVEL_BYTE] = levels[keep]
        if muzzles is not None:
            bit, col = np.uint8(SPEECH_FLAGS["muzzled"]), self._speech[:, USER_NAME_LEN + 1]
            self._speech[at, _MUZZLE_BYTE] = muzzles[keep]
            col[at] = np.where(muzzles[keep] != 0, col[at] | bit, col[at] & ~bit)
        if mesgs is not None:
            for j, p in zip(at.tolist(), keep.tolist()):
                self._afk[j] = 0
                self._afk[j, :len(mesgs[p])] = np.frombuffer(mesgs[p], dtype=np.uint8)
                self._afk[j, AFK_MESG_LEN] = len(mesgs[p])
            self._afk_dirty = True
        if descs is not None:
            for j, p in zip(at.tolist(), keep.tolist()):
                self._udesc[j] = 0
                self._udesc[j, :len(descs[p])] = np.frombuffer(descs[p], dtype=np.uint8)
                self._udesc[j, USER_DESC_LEN] = len(descs[p])
            self._udesc_dirty = True
        if logins is not None:
            self._who[at, 0] = logins[keep]
        if aways is not None:
            self._who[at, 1] = aways[keep]
        if logins is not None or aways is not None:
            self._who_dirty = True
        for f, v in phrases.items():
            first = 0 if f == "in_phrase" else _GO_OUT
            for j, p in zip(at.tolist(), keep.tolist()):
                self._go[j, first:first + PHRASE_LEN + 1] = 0
                self._go[j, first:first + len(v[p])] = np.frombuffer(v[p], dtype=np.uint8)
                self._go[j, first + PHRASE_LEN] = len(v[p])
        if invites is not None:
            self._go_invite[at] = invites[keep]
        if phrases or invites is not None:
            self._go_dirty = True
        if (names is not None or levels is not None or muzzles is not None
                or speech.keys() - {"afk", "igntell", "prompt", "charmode_echo"}):
            self._speech_dirty = True
        if speech.keys() & {"afk", "igntell"}:
            self._private_dirty = True
        if speech.keys() & {"prompt", "charmode_echo"}:
            self._set_dirty = True
        if rooms is not None or flags or not (names is not None or speech or levels is not None or muzzles is not None
                                              or mesgs is not None
                                              or descs is not None or logins is not None or aways is not None
                                              or phrases or invites is not None):
            self._dirty = True

    def table(self, rm, sender) -> np.ndarray:
        """The (capacity, 7) listener table, in LISTENER_FIELDS order, that :func:`broadcast` would take for a broadcast
        to room ``rm`` (None: every room) from slot ``sender`` (None: no sender), from the host mirror."""
        self._check_open()
        rm = _room(rm)
        sender = -1 if sender is None else self._slot(sender)
        col = LISTENER_FIELDS.index
        t = np.zeros((self.capacity, len(LISTENER_FIELDS)), dtype=np.uint8)
        for f, bit in ROSTER_FLAGS.items():
            t[:, col(f)] = (self._flags & bit) != 0
        t[:, col("has_room")] = self._room >= 0
        if rm >= 0:
            t[:, col("same_room")] = self._room == rm
        if sender >= 0:
            t[sender, col("is_sender")] = 1
        return t

    def _checked(self, broadcasts, cells: int, cells_what: str):
        """Each (text, rm, sender, force_listen, com_num) checked, after the call as a whole (``cells`` per broadcast
        must stay below 2^31 in all): the texts, their lengths, and the rooms (-1: every room), senders (-1: none),
        flags (bit 1 force_listen) and commands as lists."""
        if isinstance(broadcasts, (str, bytes, bytearray, np.ndarray)) or not hasattr(broadcasts, "__len__"):
            raise ValueError(f"broadcasts must be a sequence of tuples, not {type(broadcasts).__name__}")
        if len(broadcasts) == 0:
            raise ValueError("empty call: no broadcasts")
        if len(broadcasts) * cells >= 2**31:
            raise ValueError(f"{len(broadcasts)} broadcasts to {self.capacity} slots: {cells_what} must be below 2^31")
        texts, rms, senders, flags, coms = [], [], [], [], []
        for k, b in enumerate(broadcasts):
            if not isinstance(b, tuple) or len(b) != 5:
                raise ValueError(f"broadcast {k}: expected a (text, rm, sender, force_listen, com_num) tuple, "
                                 f"got {type(b).__name__}{f' of {len(b)}' if isinstance(b, tuple) else ''}")
            text, rm, sender, force_listen, com_num = b
            try:
                texts.append(_as_text(text))
                rms.append(_room(rm))
                senders.append(-1 if sender is None else self._slot(sender))
                flags.append(_flag("force_listen", force_listen) << 1)
                coms.append(_com_num(com_num))
            except ValueError as e:
                raise ValueError(f"broadcast {k}: {e}") from None
        lens = np.fromiter((len(t) for t in texts), dtype=np.int64, count=len(texts))
        if int(lens.sum()) >= 2**31:
            raise ValueError("call text larger than 2 GiB: split it")
        return texts, lens, rms, senders, flags, coms

    @staticmethod
    def _packed(texts, lens, rms, senders, flags, coms):
        """What _checked returns, packed for nd_roster_fanout / nd_roster_plan: texts, text offsets and lengths, rooms,
        senders, flags and commands."""
        return (b"".join(texts), _offsets(lens, np.int32), lens.astype(np.int32), np.array(rms, dtype=np.int32),
                np.array(senders, dtype=np.int32), np.array(flags, dtype=np.uint8), np.array(coms, dtype=np.int32))

    def _prepare(self, broadcasts):
        """Each (text, rm, sender, force_listen, com_num) checked, packed for nd_roster_fanout: texts, text offsets and
        lengths, rooms (-1: every room), senders (-1: none), flags (bit 1 force_listen) and commands."""
        checked = self._checked(broadcasts, self.capacity, "K x capacity")
        lens = checked[1]
        bound = int((self._room >= 0).sum()) * int((6 * lens + 4).sum())   # only a slot with a room is admitted
        if bound > MANY_ARENA_CAP:
            raise ValueError(f"call too large: its arena bound is {bound} bytes, the cap is {MANY_ARENA_CAP} "
                             f"(MANY_ARENA_CAP): split it")
        return self._packed(*checked)

    def _prepare_plan(self, broadcasts, record=None):
        """As _prepare, for nd_roster_plan: there is no arena, so its bound does not apply; the variant buffer's does
        (12 * text bytes + 16 * K at most MANY_ARENA_CAP), and K x bitmap words stays below 2^31.  ``record`` (None, one
        bool, or K of them) sets bit 2 of the flags of the broadcasts to record, each of which needs a ring room."""
        checked = self._checked(broadcasts, (self.capacity + 63) // 64, "K x ceil(capacity / 64)")
        lens = checked[1]
        bound = _variant_at(int(lens.sum()), len(lens))
        if bound > MANY_ARENA_CAP:
            raise ValueError(f"call too large: its variant bound (12 x text bytes + 16 x K) is {bound} bytes, the cap "
                             f"is {MANY_ARENA_CAP} (MANY_ARENA_CAP): split it")
        packed = self._packed(*checked)
        if record is None:
            return packed
        k, rms, flags = len(lens), checked[2], packed[5]
        if isinstance(record, (bool, np.bool_)):
            record = [record] * k
        elif isinstance(record, (str, bytes, bytearray)) or not hasattr(record, "__len__"):
            raise ValueError(f"record must be None, a bool or a sequence of one bool per broadcast, not {record!r}")
        if len(record) != k:
            raise ValueError(f"record: {len(record)} values for {k} broadcasts")
        for b, (on, rm) in enumerate(zip(record, rms)):
            if not isinstance(on, (bool, np.bool_)):
                raise ValueError(f"record must hold bools, not {on!r} (broadcast {b})")
            if not on:
                continue
            if self.review_rooms == 0:
                raise ValueError(f"broadcast {b}: it is to be recorded, but the roster has no review rings "
                                 f"(review_rooms is 0)")
            if not 0 <= rm < self.review_rooms:
                raise ValueError(f"broadcast {b}: it is to be recorded, but room {None if rm < 0 else rm} has no review "
                                 f"ring (the ring rooms are 0 .. {self.review_rooms - 1})")
            flags[b] |= _RECORD_BIT
        return packed

    def broadcast_many(self, broadcasts) -> Fanout:
        """K broadcasts to this roster in one device call: a sequence of ``(text, rm, sender, force_listen, com_num)``
        tuples, texts by :func:`broadcast`'s rules.  Item ``(k, j)`` is slot ``j`` of broadcast ``k``
        (``Fanout.item``); ``timing`` adds ``h2d_bytes`` and ``d2h_bytes``.  Malformed calls, and calls whose arena
        bound (slots with a room x the sum of max_bytes) exceeds MANY_ARENA_CAP, raise ``ValueError`` before the device
        is touched."""
        self._check_open()
        text, text_off, lens, rm, sender, flags, coms = self._prepare(broadcasts)
        lib = _load()
        handle = self._device_handle(lib)
        k = len(lens)
        m = k * self.capacity
        admitted = np.zeros(m, dtype=np.uint8)
        out_off = np.zeros(m + 1, dtype=np.int64)
        w_off = np.zeros(m + 1, dtype=np.int32)
        tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        t = _RosterTiming()
        rc = lib.nd_roster_fanout(handle, k, _ptr(tbuf), len(text), _ptr(text_off), _ptr(lens), _ptr(rm),
                                  _ptr(sender), _ptr(flags), _ptr(coms), _ptr(self._table) if self._dirty else None,
                                  _ptr(admitted), _ptr(out_off), _ptr(w_off), ctypes.byref(t))
        _check(rc, "device fan-out failed")
        self._dirty = False
        r = _result(lib, admitted, out_off, w_off, t)
        r.broadcast_offsets = np.arange(k + 1, dtype=np.int64) * self.capacity
        return r

    def _device_handle(self, lib) -> int:
        if self._handle is None:
            h = _check(lib.nd_roster_create(self.capacity), "cannot create a device roster")
            if ((self.review_rooms and lib.nd_roster_review_rooms(h, self.review_rooms) != 0)
                    or (self.revtell and lib.nd_roster_revtell_rings(h) != 0)
                    or (self.look_rooms and lib.nd_roster_look_rooms(h, self.look_rooms) != 0)
                    or (self.clones and lib.nd_roster_clones(h, self.clones) != 0)):
                lib.nd_roster_destroy(h)
                raise RuntimeError(f"cannot create a device roster: {lib.nd_last_error().decode(errors='replace')}")
            self._handle = h
        return self._handle

    def _pending_clear(self):
        """The clear bytes to send with a recording or reviewing call: a copy, or None when nothing is pending."""
        return self._clear.copy() if self._clear_pending else None

    def _clear_sent(self) -> None:
        self._clear[:] = 0
        self._clear_pending = False

    def plan_many(self, broadcasts, record=None) -> Plan:
        """The delivery plan of K broadcasts to this roster, in one device call: what :meth:`broadcast_many` takes,
        checked by the same rules, except that no arena bound applies; instead the variant bound, 12 x the call's text
        bytes + 16 x K, must not exceed MANY_ARENA_CAP.  One upload, one kernel, one download, one synchronise,
        whatever K and the capacity.  The contract::

            roster.plan_many(bs).expand() == roster.broadcast_many(bs)

        ``record`` is None, one bool for every broadcast, or K bools.  A broadcast with a true ``record`` is also
        stored in the review ring of its room ``rm``, which must be a ring room, as ``say()`` does: planned, then
        ``record(rm, text)`` -- ``np_record`` for k = 0 .. K - 1 in order, within a call and across calls.  A text of
        200 bytes or more is stored cut to 200 with a forced newline; an empty text stores an empty line.  The plan is
        the one returned without ``record``; a call that records nothing enqueues nothing more, one that does adds
        one kernel after the plan's, and no copy or synchronise."""
        self._check_open()
        text, text_off, lens, rm, sender, flags, coms = self._prepare_plan(broadcasts, record)
        recording = bool((flags & _RECORD_BIT).any())
        lib = _load()
        handle = self._device_handle(lib)
        k, words = len(lens), (self.capacity + 63) // 64
        bits = np.empty((k, words), dtype=np.uint64)
        vn = np.empty((k, 2), dtype=np.int64)
        vw = np.empty((k, 2), dtype=np.int32)
        vwsz = np.empty((k, 2, MAX_WRITES), dtype=np.int32)
        var = np.empty(_variant_at(len(text), k), dtype=np.uint8)
        tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        t = _RosterTiming()
        args = (handle, k, _ptr(tbuf), len(text), _ptr(text_off), _ptr(lens), _ptr(rm), _ptr(sender), _ptr(flags),
                _ptr(coms), _ptr(self._table) if self._dirty else None, _ptr(bits), _ptr(vn), _ptr(vw), _ptr(vwsz),
                _ptr(var), ctypes.byref(t))
        if recording:                       # the pending clears go first, with the same upload
            clear = self._pending_clear()
            rc = lib.nd_roster_plan_record(*args, _ptr(clear) if clear is not None else None)
        else:
            rc = lib.nd_roster_plan(*args)
        _check(rc, "device plan failed")
        self._dirty = False
        if recording:
            self._clear_sent()
        return Plan(capacity=self.capacity, admitted_bits=bits,
                    colour_bits=_pack((self._flags & ROSTER_FLAGS["colour"]) != 0), variants=var,
                    variant_starts=_variant_starts(text_off, lens), variant_sizes=vn, write_counts=vw,
                    write_sizes=vwsz, timing=_timing_of(t))

    def _prepare_speech(self, events, ban_swearing, record):
        """Each (slot, com, inpstr, word_count) and its speaker's state checked, packed for nd_roster_speak: the inpstr,
        their offsets and lengths, the slots, commands and word counts, the two flags, and whether the call records."""
        if isinstance(events, (str, bytes, bytearray, np.ndarray)) or not hasattr(events, "__len__"):
            raise ValueError(f"events must be a sequence of tuples, not {type(events).__name__}")
        if len(events) == 0:
            raise ValueError("empty call: no events")
        ban_swearing, record = _flag("ban_swearing", ban_swearing), _flag("record", record)
        if len(events) * self.capacity >= 2**31 - 1:
            raise ValueError(f"{len(events)} events to {self.capacity} slots: K x capacity must be below 2^31 - 1")
        texts, slots, coms, wcs = [], [], [], []
        recording = False
        for k, ev in enumerate(events):
            if not isinstance(ev, tuple) or len(ev) != 4:
                raise ValueError(f"event {k}: expected a (slot, com, inpstr, word_count) tuple, "
                                 f"got {type(ev).__name__}{f' of {len(ev)}' if isinstance(ev, tuple) else ''}")
            slot, com, inpstr, wc = ev
            try:
                slot = self._slot(slot)
                if not _is_int(com, 0, NUM_COMMANDS - 1) or int(com) not in _SPEECH_COMS:
                    raise ValueError(f"com must be COM_SAY, COM_SHOUT, COM_EMOTE or COM_SEMOTE "
                                     f"({', '.join(map(str, _SPEECH_COMS))}), not {com!r}")
                text = _as_text(inpstr)
                if len(text) >= ARR_SIZE:
                    raise ValueError(f"inpstr of {len(text)} bytes: the talker's input line holds at most {ARR_SIZE - 1}")
                if not _is_int(wc, 0, MAX_WORDS):
                    raise ValueError(f"word_count must be an int in [0, {MAX_WORDS}], not {wc!r}")
                to_record = bool(record and _SPEECH_COMS[int(com)])
                self._check_speaker(slot, "it is to be recorded" if to_record else None)
                recording |= to_record
            except ValueError as e:
                raise ValueError(f"event {k}: {e}") from None
            texts.append(text)
            slots.append(slot)
            coms.append(int(com))
            wcs.append(int(wc))
        lens = np.fromiter((len(t) for t in texts), dtype=np.int64, count=len(texts))
        bound = _variant_at(_composed_at(2 * int(lens.sum()), 2 * len(lens)), 2 * len(lens))
        if bound > MANY_ARENA_CAP:
            raise ValueError(f"call too large: its variant bound is {bound} bytes, the cap is {MANY_ARENA_CAP} "
                             f"(MANY_ARENA_CAP): split it")
        return (b"".join(texts), _offsets(lens, np.int32), lens.astype(np.int32), np.array(slots, dtype=np.int32),
                np.array(coms, dtype=np.uint8), np.array(wcs, dtype=np.uint8), ban_swearing, recording)

    def speak_many(self, events, ban_swearing=False, record=False) -> Speech:
        """K speech events in one device call: a non-empty sequence of ``(slot, com, inpstr, word_count)`` tuples, what
        the talker's ``say()``, ``shout()``, ``emote()`` and ``semote()`` receive (nuts333.c:4062-4226).  ``com`` is
        COM_SAY, COM_SHOUT, COM_EMOTE or COM_SEMOTE; ``inpstr`` is a text by :func:`broadcast`'s rules of at most 999
        bytes -- ``.shout X`` passes ``X``, a plain line the whole line, the ``;x`` / ``#x`` shortcuts the whole line
        with its first byte; ``word_count`` is the talker's, an int in [0, 10].  The speaker must have a room, a name
        and no ``login`` flag.  Anything else raises ``ValueError("event k: ...")`` before the device is touched.

        The device decides each event's outcome in the reference's order: MUZZLED if the speaker is muzzled; NOTHING if
        ``word_count < 2`` and, for a say, ``command_mode``, for an emote or semote, byte 1 of ``inpstr`` as a signed
        char below 33; SWEARING if ``ban_swearing`` and the text holds a swear word (not for a semote, which the
        reference does not check); else SPOKEN.  In the NOTHING test byte 1 of an ``inpstr`` shorter than 2 bytes counts
        as 0: the reference reads a stale byte of its input buffer there.  Returns a :class:`Speech`; for every spoken
        event ``k`` its ``room`` plan at ``k`` is ``plan_many([(speech.line(k), rm, sender, 0, com)])`` at 0, with
        ``(rm, sender)`` the speaker's room and slot for a say, ``(None, slot)`` for a shout, ``(room, None)`` for an
        emote and ``(None, None)`` for a semote.

        ``record=True`` stores every spoken say and emote in its speaker's room ring as ``plan_many(record=)`` stores a
        line, in event order, after the pending ``clear_review``; every say and emote event's speaker must then be in a
        ring room, whatever its outcome turns out to be.  Shouts and semotes are never recorded.

        One upload (the table and the speaker state only after an update of theirs), two kernel launches
        (nuts_roster_speak, nuts_roster_speak_plan) -- three in a call that records (nuts_roster_record) --, one
        download at the bound size and one synchronise, whatever K and the capacity."""
        self._check_open()
        text, text_off, lens, slots, coms, wcs, ban, recording = self._prepare_speech(events, ban_swearing, record)
        lib = _load()
        handle = self._device_handle(lib)
        k = len(lens)
        out = self._speech_arrays(k, len(text))
        tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        clear = self._pending_clear() if recording else None
        t = _RosterTiming()
        rc = lib.nd_roster_speak(handle, k, _ptr(tbuf), len(text), _ptr(text_off), _ptr(lens), _ptr(slots), _ptr(coms),
                                 _ptr(wcs), ban, int(recording), _ptr(self._table) if self._dirty else None,
                                 _ptr(self._speech) if self._speech_dirty else None,
                                 _ptr(clear) if clear is not None else None, *map(_ptr, out), ctypes.byref(t))
        _check(rc, "device speech failed")
        self._private_dirty &= not self._speech_dirty      # the whole speaker mirror went up, or none of it
        self._dirty = self._speech_dirty = False
        if recording:
            self._clear_sent()
        return self._speech_of(len(text), text_off, slots, *out, t)

    def _speech_arrays(self, k: int, text_bytes: int):
        """The arrays nd_roster_speak / nd_roster_input fill in for k events over text_bytes of inpstr or reads, in the
        library's order and as _speech_of takes them: outcome, clen, bits, vn, vw, vwsz, ctext, var."""
        ctext_bytes = _composed_at(2 * text_bytes, 2 * k)
        return (np.empty(k, dtype=np.int8), np.empty((2, k), dtype=np.int32),
                np.empty((k, (self.capacity + 63) // 64), dtype=np.uint64), np.empty((2, k, 2), dtype=np.int64),
                np.empty((2, k, 2), dtype=np.int32), np.empty((2, k, 2, MAX_WRITES), dtype=np.int32),
                np.empty(ctext_bytes, dtype=np.uint8), np.empty(_variant_at(ctext_bytes, 2 * k), dtype=np.uint8))

    def _speech_of(self, text_bytes, text_off, slots, outcome, clen, bits, vn, vw, vwsz, ctext, var, t) -> Speech:
        """The Speech of what nd_roster_speak / nd_roster_input filled in."""
        k, words = len(slots), (self.capacity + 63) // 64
        # text t = k is event k's room line, K + k its reply
        at = text_off.astype(np.int64)
        tstarts = np.stack([_composed_at(at, np.arange(k)), _composed_at(text_bytes + at, k + np.arange(k))])
        starts = _variant_starts(tstarts, clen)
        reply_bits = np.zeros((k, words), dtype=np.uint64)
        has = np.flatnonzero(clen[1] >= 0)
        reply_bits[has, slots[has] // 64] = np.uint64(1) << (slots[has] % 64).astype(np.uint64)
        timing = _timing_of(t)
        colour_bits = _pack((self._flags & ROSTER_FLAGS["colour"]) != 0)
        plans = [Plan(capacity=self.capacity, admitted_bits=b, colour_bits=colour_bits, variants=var,
                      variant_starts=starts[i], variant_sizes=vn[i], write_counts=vw[i], write_sizes=vwsz[i],
                      timing=dict(timing)) for i, b in enumerate((bits, reply_bits))]
        return Speech(outcome=outcome, room=plans[0], reply=plans[1], texts=ctext, text_starts=tstarts,
                      text_sizes=clen.astype(np.int64), timing=timing)

    def _prepare_input(self, reads, ban_swearing, record):
        """Each (slot, data) and its speaker's state checked, packed for nd_roster_input: the reads as given, their
        bytes, offsets and lengths, the slots, the two flags."""
        if isinstance(reads, (str, bytes, bytearray, np.ndarray)) or not hasattr(reads, "__len__"):
            raise ValueError(f"reads must be a sequence of tuples, not {type(reads).__name__}")
        if len(reads) == 0:
            raise ValueError("empty call: no reads")
        ban_swearing, record = _flag("ban_swearing", ban_swearing), _flag("record", record)
        if len(reads) * self.capacity >= 2**31 - 1:
            raise ValueError(f"{len(reads)} reads to {self.capacity} slots: K x capacity must be below 2^31 - 1")
        datas, slots = [], []
        for k, rd in enumerate(reads):
            if not isinstance(rd, tuple) or len(rd) != 2:
                raise ValueError(f"read {k}: expected a (slot, data) tuple, "
                                 f"got {type(rd).__name__}{f' of {len(rd)}' if isinstance(rd, tuple) else ''}")
            try:
                slot = self._slot(rd[0])
                data = _read_data(rd[1])
                # which reads are says and emotes, the device decides
                self._check_speaker(slot, "it may be recorded" if record else None)
            except ValueError as e:
                raise ValueError(f"read {k}: {e}") from None
            datas.append(data)
            slots.append(slot)
        lens = np.fromiter((len(d) for d in datas), dtype=np.int64, count=len(datas))
        bound = _variant_at(_composed_at(2 * int(lens.sum()), 2 * len(lens)), 2 * len(lens))
        if bound > MANY_ARENA_CAP:
            raise ValueError(f"call too large: its variant bound is {bound} bytes, the cap is {MANY_ARENA_CAP} "
                             f"(MANY_ARENA_CAP): split it")
        return (datas, b"".join(datas), _offsets(lens, np.int32), lens.astype(np.int32),
                np.array(slots, dtype=np.int32), ban_swearing, record)

    def input_many(self, reads, ban_swearing=False, record=False) -> Input:
        """K reads of clients in line mode in one device call: a non-empty sequence of ``(slot, data)`` tuples, what
        ``user_input()`` gets from ``read(2)`` (nuts333.c:136-235).  ``data`` is bytes, bytearray, memoryview or a
        latin-1 str of 1 .. READ_SIZE bytes of any value, NUL included, whose last byte is below 32 as a signed char;
        a read that does not end so belongs to ``get_charclient_line``, whose per-user buffer the roster does not keep.
        The speaker must have a room, a name and no ``login`` flag, as for :meth:`speak_many`.  Anything else raises
        ``ValueError("read k: ...")`` before the device is touched.

        The device does, per read and in the reference's order: ``data[0] == 255`` is IAC and nothing else happens; the
        line is ``data`` up to its first byte below 32 as a signed char (``np_terminate``); it is split as
        ``np_wordfind`` splits it, a run of more than 39 bytes counting as several words and ten or more words as nine;
        ``.`` alone is REPEAT; a line without a word is EMPTY; a speaker not in ``command_mode`` whose line does not
        begin with one of ``.;!<>-#`` says the whole line; otherwise ``exec_com``'s front part (nuts333.c:3753-3785)
        finds the command -- ``comword`` is the first word without one leading ``.``, the words ``>``, ``<``, ``-`` and
        ``!`` are tell, pemote, echo and shout, a line that begins with ``;`` or ``#`` is an emote or semote of the
        whole line, and else the first of the 92 names that begins with ``comword`` wins and ``inpstr`` starts at the
        second word (``np_remove_first``).  No command, or one above the speaker's ``level``, is UNKNOWN; say, shout,
        emote and semote are SPEECH, answered as :meth:`speak_many` answers ``(slot, com, inpstr, word_count)``; every
        other command is COMMAND and left to the caller.  A say through ``exec_com`` with fewer than two words is
        answered ``Say what?`` before the muzzle is looked at, whatever the mode (nuts333.c:3826-3829).

        ``record=True`` records as ``speak_many(record=True)`` does.  Which reads are says and emotes is decided on the
        device, so every speaker must then stand in a ring room.

        One upload (the table and the speaker state only after an update of theirs), three kernel launches
        (nuts_roster_parse, nuts_roster_speak, nuts_roster_speak_plan) -- four in a call that records
        (nuts_roster_record) --, one download at the bound size and one synchronise, whatever K and the capacity.  A
        composed text's slot in the text buffer is ``len(data) + 36`` bytes wide."""
        self._check_open()
        datas, data, off, lens, slots, ban, record = self._prepare_input(reads, ban_swearing, record)
        lib = _load()
        handle = self._device_handle(lib)
        k = len(lens)
        kind, com = np.empty(k, dtype=np.int8), np.empty(k, dtype=np.int8)
        wcs = np.empty(k, dtype=np.uint8)
        line_len, inp_off, inp_len = (np.empty(k, dtype=np.int32) for _ in range(3))
        out = self._speech_arrays(k, len(data))
        dbuf = np.frombuffer(data, dtype=np.uint8)
        clear = self._pending_clear() if record else None
        t = _RosterTiming()
        rc = lib.nd_roster_input(handle, k, _ptr(dbuf), len(data), _ptr(off), _ptr(lens), _ptr(slots), ban, record,
                                 _ptr(self._table) if self._dirty else None,
                                 _ptr(self._speech) if self._speech_dirty else None,
                                 _ptr(clear) if clear is not None else None, _ptr(kind), _ptr(com), _ptr(wcs),
                                 _ptr(line_len), _ptr(inp_off), _ptr(inp_len), *map(_ptr, out), ctypes.byref(t))
        _check(rc, "device input failed")
        self._private_dirty &= not self._speech_dirty
        self._dirty = self._speech_dirty = False
        if record:
            self._clear_sent()
        speech = self._speech_of(len(data), off, slots, *out, t)
        return Input(kind=kind, com=com, word_count=wcs, line_sizes=line_len, inpstr_starts=inp_off.astype(np.int64),
                     inpstr_sizes=inp_len.astype(np.int64), speech=speech, data=datas, timing=dict(speech.timing))

    def _prepare_private(self, events, record):
        """Each (slot, com, inpstr, word_count) and its speaker's state checked as _prepare_speech checks them, packed for
        nd_roster_tell: the inpstr, their offsets and lengths, the slots, commands and word counts, and the flag."""
        if isinstance(events, (str, bytes, bytearray, np.ndarray)) or not hasattr(events, "__len__"):
            raise ValueError(f"events must be a sequence of tuples, not {type(events).__name__}")
        if len(events) == 0:
            raise ValueError("empty call: no events")
        record = _flag("record", record)
        if record and not self.revtell:
            raise ValueError("record: the roster has no revtell rings (revtell is False)")
        if len(events) * self.capacity >= 2**31 - 1:
            raise ValueError(f"{len(events)} events to {self.capacity} slots: K x capacity must be below 2^31 - 1")
        texts, slots, coms, wcs = [], [], [], []
        for k, ev in enumerate(events):
            if not isinstance(ev, tuple) or len(ev) != 4:
                raise ValueError(f"event {k}: expected a (slot, com, inpstr, word_count) tuple, "
                                 f"got {type(ev).__name__}{f' of {len(ev)}' if isinstance(ev, tuple) else ''}")
            slot, com, inpstr, wc = ev
            try:
                slot = self._slot(slot)
                if not _is_int(com, 0, NUM_COMMANDS - 1) or int(com) not in (COM_TELL, COM_PEMOTE):
                    raise ValueError(f"com must be COM_TELL or COM_PEMOTE ({COM_TELL}, {COM_PEMOTE}), not {com!r}")
                text = _as_text(inpstr)
                if len(text) >= ARR_SIZE:
                    raise ValueError(f"inpstr of {len(text)} bytes: the talker's input line holds at most {ARR_SIZE - 1}")
                if not _is_int(wc, 0, MAX_WORDS):
                    raise ValueError(f"word_count must be an int in [0, {MAX_WORDS}], not {wc!r}")
                self._check_speaker(slot, None)
            except ValueError as e:
                raise ValueError(f"event {k}: {e}") from None
            texts.append(text)
            slots.append(slot)
            coms.append(int(com))
            wcs.append(int(wc))
        lens = np.fromiter((len(t) for t in texts), dtype=np.int64, count=len(texts))
        bound = _variant_at(_composed_at(2 * int(lens.sum()), 2 * len(lens), _TELL_SLACK), 2 * len(lens))
        if bound > MANY_ARENA_CAP:
            raise ValueError(f"call too large: its variant bound is {bound} bytes, the cap is {MANY_ARENA_CAP} "
                             f"(MANY_ARENA_CAP): split it")
        return (b"".join(texts), _offsets(lens, np.int32), lens.astype(np.int32), np.array(slots, dtype=np.int32),
                np.array(coms, dtype=np.uint8), np.array(wcs, dtype=np.uint8), record)

    def tell_many(self, events, record=False) -> Private:
        """K private speech events in one device call: a non-empty sequence of ``(slot, com, inpstr, word_count)``
        tuples, what the talker's ``tell()`` and ``pemote()`` receive (nuts333.c:4128-4182, 4230-4281), shaped and
        checked as :meth:`speak_many` checks them.  ``com`` is COM_TELL or COM_PEMOTE; ``inpstr`` is the line without
        its first word, ``"bobby hello"`` for ``.tell bobby hello`` and for ``> bobby hello`` -- what a COMMAND read
        of :meth:`input_many` with ``com`` 5 or 8 hands back.  There is no ``ban_swearing``: the reference does not
        check tells.  Anything malformed raises ``ValueError("event k: ...")`` before the device is touched.

        The device does, per event and in the reference's order: ``word[1]`` is the first word of ``inpstr`` as
        ``np_wordfind`` finds it (leading bytes below 33 as signed chars skipped, the run of bytes above 32 cut at 39),
        its first byte capitalised if it is a-z.  A tell is MUZZLED if the speaker is muzzled, NOTHING if
        ``word_count < 3``, NOBODY if ``get_user`` finds nobody, SELF if it finds the speaker, then ``private_blocked``,
        else TOLD.  A pemote is MUZZLED, NOTHING, SELF if the capitalised word equals the speaker's name exactly, NOBODY,
        ``private_blocked``, else TOLD -- one that reaches the speaker through a substring match goes to the speaker
        itself, as in the reference.  ``get_user`` runs over the slots in ascending order, skipping those with the
        ``login`` flag or without a name: the lowest slot whose name equals the word, else the lowest whose name
        contains it; a slot without a room is found, and answered OFFSITE.  ``private_blocked`` is AFK (with or without
        the target's message), IGNALL and IGNTELL (the target's flag, and the speaker's level below 2 or below the
        target's), OFFSITE.  A TOLD event composes the speaker's echo and the target's line from
        ``np_remove_first(inpstr)``; every other outcome the one notice.  Returns a :class:`Private`; for a TOLD event
        ``told.chunks(k, c) == plan_many([(private.line(k), None, None, 0, com)]).chunks(0, c)``, and ``reply`` likewise.

        ``record=True`` needs ``Roster(..., revtell=True)`` and stores every TOLD event's line in its target's revtell
        ring as ``np_record(ring, 5, &revline, line)`` does, in event order within a call and across calls, after the
        pending :meth:`clear_revtell`; a line of 200 bytes or more is cut with the forced newline.

        One upload (the table, the speaker state and the AFK messages only after an update of theirs), two kernel
        launches (nuts_roster_tell, nuts_roster_speak_plan) -- three in a call that records (nuts_roster_record_tell)
        --, one download at the bound size and one synchronise, whatever K and the capacity.  A composed text's slot in
        the text buffer is ``len(inpstr) + 96`` bytes wide.

        Out of scope: routing inside ``input_many`` (feed its COMMAND reads with ``com`` 5 or 8 here); the "is using
        the editor" wording of the ignall notice (the roster has no editor state, and oracle/talker_port.c omits it
        too); remote (``T_REMOTE``) targets and clones; the prompt; ``.afk`` and ``.igntell`` themselves -- the caller
        updates the fields."""
        self._check_open()
        text, text_off, lens, slots, coms, wcs, record = self._prepare_private(events, record)
        lib = _load()
        handle = self._device_handle(lib)
        k, words = len(lens), (self.capacity + 63) // 64
        ctext_bytes = _composed_at(2 * len(text), 2 * k, _TELL_SLACK)
        outcome, target = np.empty(k, dtype=np.int8), np.empty(k, dtype=np.int32)
        clen = np.empty((2, k), dtype=np.int32)
        vn, vw = np.empty((2, k, 2), dtype=np.int64), np.empty((2, k, 2), dtype=np.int32)
        vwsz = np.empty((2, k, 2, MAX_WRITES), dtype=np.int32)
        ctext = np.empty(ctext_bytes, dtype=np.uint8)
        var = np.empty(_variant_at(ctext_bytes, 2 * k), dtype=np.uint8)
        tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        clear = self._tell_clear.copy() if record and self._tell_clear_pending else None
        t = _RosterTiming()
        rc = lib.nd_roster_tell(handle, k, _ptr(tbuf), len(text), _ptr(text_off), _ptr(lens), _ptr(slots), _ptr(coms),
                                _ptr(wcs), record, _ptr(self._table) if self._dirty else None,
                                _ptr(self._speech) if self._speech_dirty or self._private_dirty else None,
                                _ptr(self._afk) if self._afk_dirty else None,
                                _ptr(clear) if clear is not None else None, _ptr(outcome), _ptr(target), _ptr(clen),
                                _ptr(vn), _ptr(vw), _ptr(vwsz), _ptr(ctext), _ptr(var), ctypes.byref(t))
        _check(rc, "device private speech failed")
        self._dirty = self._speech_dirty = self._private_dirty = self._afk_dirty = False
        if record:
            self._tell_clear_sent()
        at = text_off.astype(np.int64)
        tstarts = np.stack([_composed_at(at, np.arange(k), _TELL_SLACK),
                            _composed_at(len(text) + at, k + np.arange(k), _TELL_SLACK)])
        starts = _variant_starts(tstarts, clen)
        bits = np.zeros((2, k, words), dtype=np.uint64)            # the target alone, the speaker alone
        for row, who in enumerate((target, slots)):
            has = np.flatnonzero(clen[row] >= 0)
            bits[row, has, who[has] // 64] = np.uint64(1) << (who[has] % 64).astype(np.uint64)
        timing = _timing_of(t)
        colour_bits = _pack((self._flags & ROSTER_FLAGS["colour"]) != 0)
        plans = [Plan(capacity=self.capacity, admitted_bits=bits[i], colour_bits=colour_bits, variants=var,
                      variant_starts=starts[i], variant_sizes=vn[i], write_counts=vw[i], write_sizes=vwsz[i],
                      timing=dict(timing)) for i in (0, 1)]
        return Private(outcome=outcome, target=target, told=plans[0], reply=plans[1], texts=ctext, text_starts=tstarts,
                       text_sizes=clen.astype(np.int64), timing=timing)

    def _look_room(self, v) -> int:
        if not _is_int(v, 0, self.look_rooms - 1):
            raise ValueError(f"room {v!r} has no room record: " + (f"the look rooms are 0 .. {self.look_rooms - 1}"
                             if self.look_rooms else "the roster has none (look_rooms is 0)"))
        return int(v)

    def set_rooms(self, rooms, *, name=_KEEP, access=_KEEP, desc=_KEEP, links=_KEEP, topic=_KEEP, mesg_cnt=_KEEP,
                  netlink=_KEEP, inlink=_KEEP) -> None:
        """Set fields of the room records of ``rooms`` (a look room or a sequence of them), by the conventions of
        :meth:`update`: each field given is one value for every room or a sequence of one per room, a field not given
        stays as it is, a room given more than once takes its last values, and nothing changes unless the whole call
        is valid (``ValueError("room N: ...")`` names the first bad entry's position).  Like ``update`` it does not touch
        the device; :meth:`look_many`, :meth:`who_many` and :meth:`rooms_many` upload the room table, whichever comes first.

        ``name`` is at most ROOM_NAME_LEN bytes, ``access`` PUBLIC, PRIVATE, FIXED_PUBLIC or FIXED_PRIVATE (0 .. 3),
        ``desc`` at most ROOM_DESC_LEN bytes and may hold newlines, ``links`` at most MAX_LINKS look rooms in the order
        ``look()`` lists them (one list of ints is one value for every room), ``topic`` at most TOPIC_LEN bytes (empty:
        none set), ``mesg_cnt`` the board's message count in [0, 2^31), and ``netlink`` None, or ``(service, allow_in)``
        for a room whose netlink is UP: a service name of at most SERV_NAME_LEN bytes and whether the link allows
        incoming users only (nuts333.c:3966-3970).  ``netlink`` may also be ``(service, allow_in, state)`` with LINK_DOWN
        (the link is unconnected), LINK_VERIFYING (connected, not yet up) or LINK_UP: ``.rmsn`` tells the three apart and
        prints the service of each (c:5684-5694), while ``look()``, ``who()`` and ``update(away=)`` know a link only when
        it is UP.  ``inlink`` (a bool, False at first) is ``rm->inlink``, which ``.rmsn`` prints.  The texts are bytes or
        str, one byte per character, without a NUL."""
        self._check_open()
        if isinstance(rooms, (int, np.integer)):
            rooms = [rooms]
        if isinstance(rooms, (str, bytes, bytearray)) or not hasattr(rooms, "__len__"):
            raise ValueError(f"rooms must be a look room or a sequence of them, not {rooms!r}")
        idx = np.array([self._look_room(v) for v in rooms], dtype=np.int64)
        n = len(idx)

        def numbered(what, v, conv, scalar):
            """As _one_or_each, a bad entry reported by its position."""
            if scalar(v):
                try:
                    return [conv(v)] * n
                except ValueError as e:
                    raise ValueError(f"room 0: {e}") from None
            if _is_text(v) or not hasattr(v, "__len__"):
                raise ValueError(f"{what} must be a value or a sequence of one per room, not {v!r}")
            if len(v) != n:
                raise ValueError(f"{what}: {len(v)} values for {n} rooms")
            out = []
            for i, x in enumerate(v):
                try:
                    out.append(conv(x))
                except ValueError as e:
                    raise ValueError(f"room {i}: {e}") from None
            return out

        def access_of(v):
            if not _is_int(v, 0, 3):
                raise ValueError(f"access must be PUBLIC, PRIVATE, FIXED_PUBLIC or FIXED_PRIVATE (0 .. 3), not {v!r}")
            return int(v)

        def links_of(v):
            if _is_text(v) or not hasattr(v, "__len__") or len(v) > MAX_LINKS:
                raise ValueError(f"links must be a sequence of at most {MAX_LINKS} look rooms, not {v!r}")
            return [self._look_room(x) for x in v]

        def count_of(v):
            if not _is_int(v, 0, 2**31 - 1):
                raise ValueError(f"mesg_cnt must be an int in [0, 2^31), not {v!r}")
            return int(v)

        def netlink_of(v):
            if v is None:
                return None
            if not isinstance(v, tuple) or len(v) not in (2, 3) or not isinstance(v[1], (bool, np.bool_)):
                raise ValueError(f"netlink must be None or a (service, allow_in: bool[, state]) tuple, not {v!r}")
            state = v[2] if len(v) == 3 else LINK_UP
            if isinstance(state, (bool, np.bool_)) or not _is_int(state, LINK_DOWN, LINK_UP):
                raise ValueError(f"a netlink's state must be LINK_DOWN, LINK_VERIFYING or LINK_UP (0 .. 2), not {state!r}")
            return _limited_text("netlink service", v[0], SERV_NAME_LEN), bool(v[1]), _NET_STATE[int(state)]

        def inlink_of(v):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"inlink must be a bool, not {v!r}")
            return bool(v)

        text_of = lambda what, most: (lambda v: _limited_text(what, v, most))
        new = {}
        for what, v, conv, scalar in (
                ("name", name, text_of("name", ROOM_NAME_LEN), _is_text), ("access", access, access_of, _is_number),
                ("desc", desc, text_of("desc", ROOM_DESC_LEN), _is_text),
                ("links", links, links_of, lambda v: hasattr(v, "__len__") and not _is_text(v) and all(_is_number(x) for x in v)),
                ("topic", topic, text_of("topic", TOPIC_LEN), _is_text), ("mesg_cnt", mesg_cnt, count_of, _is_number),
                ("netlink", netlink, netlink_of, lambda v: v is None or (isinstance(v, tuple) and len(v) in (2, 3) and _is_text(v[0]))),
                ("inlink", inlink, inlink_of, lambda v: not hasattr(v, "__len__"))):
            if v is not _KEEP:
                new[what] = numbered(what, v, conv, scalar)
        rec, rows = self._room_rec, self._room_desc

        def put(row, at, text, len_at, most):
            row[at:at + most] = 0
            row[at:at + len(text)] = np.frombuffer(text, dtype=np.uint8)
            row[len_at] = len(text)

        for p, j in enumerate(idx.tolist()):                  # in order: the last value wins
            if "name" in new:
                put(rec[j], 0, new["name"][p], 20, ROOM_NAME_LEN)
            if "access" in new:
                rec[j, 21] = new["access"][p]
            if "links" in new:
                rec[j, 22] = len(new["links"][p])
                rec[j, 32:72] = 0
                rec[j, 32:32 + 4 * len(new["links"][p])] = np.array(new["links"][p], dtype="<i4").view(np.uint8)
            if "topic" in new:
                put(rec[j], 72, new["topic"][p], 23, TOPIC_LEN)
            if "netlink" in new:
                link = new["netlink"][p]
                put(rec[j], 132, link[0] if link else b"", 25, SERV_NAME_LEN)
                rec[j, 24] = (int(rec[j, 24]) & _NET_INLINK) | ((link[2] | (_NET_ALLOW_IN if link[1] else 0)) if link else 0)
            if "inlink" in new:
                rec[j, 24] = (int(rec[j, 24]) & ~_NET_INLINK) | (_NET_INLINK if new["inlink"][p] else 0)
            if "mesg_cnt" in new:
                rec[j, 28:32] = np.array([new["mesg_cnt"][p]], dtype="<i4").view(np.uint8)
            if "desc" in new:
                rows[j] = 0
                rows[j, :len(new["desc"][p])] = np.frombuffer(new["desc"][p], dtype=np.uint8)
                rec[j, 26:28] = np.array([len(new["desc"][p])], dtype="<u2").view(np.uint8)
        if new and n:
            self._rooms_dirty = True

    def look_many(self, slots) -> Look:
        """What ``look()`` writes for each of ``slots``, K >= 1 lookers (duplicates allowed), in one device call
        (nuts333.c:3942-4004).  Each looker needs a room with a room record, one in ``[0, look_rooms)``; otherwise the
        call raises ``ValueError("look N: ...")`` before the device is touched.  The ``login`` flag is not consulted:
        ``connect_user`` looks while it is still set.  The looker's level and colour are those in the roster.

        For looker ``u`` in room ``rm`` the :class:`Look` holds, in order, what these ``write_user`` calls send, each
        string transduced on its own with ``u``'s colour flag (an empty string, and the trailing reset with colour on,
        are writes too): ``"\\n~FTRoom: ~FR|~FG<name>\\n\\n"``; the room's ``desc``; the exits -- the links with ``~FR`` /
        ``~FG`` by each linked room's ``access & PRIVATE``, then the netlink's service with ``*`` (``~FR`` when
        ``allow_in``), ``"\\n~FTThere are no exits."`` when there is neither --; ``"~FTYou can see:\\n"`` and a line per
        member, or ``"~FTYou are all alone here.\\n"``; ``"\\n"``; the access sentence with the board's message count;
        the topic, or ``"No topic has been set yet.\\n"``.  A member is a slot ``j != u``, ascending, with ``room[j] ==
        rm``, a name, and ``vis[j] or level[j] <= level[u]``; its line is ``"      %s %s~RS  %s\\n"`` of name, desc and
        ``~BR(AFK)`` or nothing, ``"     ~FR*~RS%s %s~RS  %s\\n"`` when it is invisible.  A slot without a name is not a
        user, as in :meth:`tell_many`: the talker's user list holds no such entry.  ``login`` slots of the room are
        listed, as the reference lists them once they have a room.

        One upload (the table, the speaker state, the room table and the descriptions only after an update of theirs),
        two kernel launches (nuts_roster_look, nuts_roster_speak_plan), one download at the bound size and one
        synchronise, whatever K and the capacity.  The bound counts a line per slot of the call's distinct rooms and a
        member per such slot and looker; a call whose variant bound exceeds MANY_ARENA_CAP is refused.

        Out of scope: clones and remote users in the list.  ``.who`` is :meth:`who_many`, ``.go`` :meth:`go_many`."""
        self._check_open()
        if isinstance(slots, (str, bytes, bytearray)) or not hasattr(slots, "__len__"):
            raise ValueError(f"slots must be a sequence of slots, not {slots!r}")
        if len(slots) == 0:
            raise ValueError("empty call: no lookers")
        if len(slots) * self.capacity >= 2**31 - 1:
            raise ValueError(f"{len(slots)} looks at {self.capacity} slots: K x capacity must be below 2^31 - 1")
        lookers, room_index, rooms = [], [], {}
        for k, v in enumerate(slots):
            try:
                u = self._slot(v)
                if not 0 <= self._room[u] < self.look_rooms:
                    raise ValueError(f"the looker, slot {u}, is in " + (f"room {int(self._room[u])}, which has no room record"
                                     if self._room[u] >= 0 else "no room") + f" (look_rooms is {self.look_rooms})")
            except ValueError as e:
                raise ValueError(f"look {k}: {e}") from None
            lookers.append(u)
            room_index.append(rooms.setdefault(int(self._room[u]), len(rooms)))
        k, nr = len(lookers), len(rooms)
        rms = np.array(list(rooms), dtype=np.int32)
        population = np.array([int((self._room == rm).sum()) for rm in rooms], dtype=np.int64)
        line_off = _offsets(population, np.int64, total=True)
        lroom = np.array(room_index, dtype=np.int32)
        m_off = _offsets(population[lroom], np.int64, total=True)
        nl, nm = int(line_off[-1]), int(m_off[-1])
        texts = 5 * nr + 3 + nl
        ctext_bytes = _LOOK_STRIDE * nr + _LOOK_FIXED_STRIDE + _LINE_ROW * nl
        bound = _variant_at(ctext_bytes, texts) + 8 * nm
        if bound > MANY_ARENA_CAP:
            raise ValueError(f"call too large: its variant and member bound is {bound} bytes, the cap is {MANY_ARENA_CAP} "
                             f"(MANY_ARENA_CAP): split it")
        lib = _load()
        handle = self._device_handle(lib)
        slot_arr = np.array(lookers, dtype=np.int32)
        line_off32, m_off32 = line_off.astype(np.int32), m_off.astype(np.int32)
        nmem, nline = np.empty(k, dtype=np.int32), np.empty(nr, dtype=np.int32)
        clen = np.empty(texts, dtype=np.int32)
        vn, vw = np.empty((texts, 2), dtype=np.int64), np.empty((texts, 2), dtype=np.int32)
        vwsz = np.empty((texts, 2, MAX_WRITES), dtype=np.int32)
        ctext = np.empty(ctext_bytes, dtype=np.uint8)
        var = np.empty(_variant_at(ctext_bytes, texts), dtype=np.uint8)
        members, mline = np.empty(max(nm, 1), dtype=np.int32), np.empty(max(nm, 1), dtype=np.int32)
        line_slot = np.full(max(nl, 1), -1, dtype=np.int32)
        t = _RosterTiming()
        rc = lib.nd_roster_look(handle, k, _ptr(slot_arr), _ptr(lroom), nr, _ptr(rms), _ptr(line_off32), _ptr(m_off32),
                                _ptr(self._table) if self._dirty else None,
                                _ptr(self._speech) if self._speech_dirty or self._private_dirty else None,
                                _ptr(self._rooms) if self._rooms_dirty else None,
                                _ptr(self._udesc) if self._udesc_dirty else None, _ptr(nmem), _ptr(nline), _ptr(clen),
                                _ptr(vn), _ptr(vw), _ptr(vwsz), _ptr(ctext), _ptr(var), _ptr(members), _ptr(mline),
                                _ptr(line_slot), ctypes.byref(t))
        _check(rc, "device look failed")
        self._dirty = self._speech_dirty = self._private_dirty = self._rooms_dirty = self._udesc_dirty = False
        tstarts = np.concatenate([
            (_LOOK_STRIDE * np.arange(nr, dtype=np.int64)[:, None] + np.array(_LOOK_TEXT_AT, dtype=np.int64)).ravel(),
            _LOOK_STRIDE * nr + np.array(_LOOK_FIXED_AT, dtype=np.int64),
            _LOOK_STRIDE * nr + _LOOK_FIXED_STRIDE + _LINE_ROW * np.arange(nl, dtype=np.int64)])
        for i in range(nr):                                     # the lines past a room's count are nobody's
            line_slot[int(line_off[i]) + int(nline[i]):int(line_off[i + 1])] = -1
        return Look(slots=slot_arr, colour=((self._flags[slot_arr] & ROSTER_FLAGS["colour"]) != 0).astype(np.uint8),
                    room_index=lroom, rooms=rms, member_slots=members[:nm], member_lines=mline[:nm],
                    member_starts=m_off[:-1].copy(), member_counts=nmem, line_slots=line_slot[:nl], texts=ctext,
                    text_starts=tstarts, text_sizes=clen.astype(np.int64), variants=var,
                    variant_starts=_variant_starts(tstarts, clen), variant_sizes=vn, write_counts=vw, write_sizes=vwsz,
                    timing=_timing_of(t))

    def who_many(self, slots, *, now, date) -> Who:
        """What ``who(user, 0)`` writes for each of ``slots``, K >= 1 lookers (duplicates allowed), in one device call
        (nuts333.c:4792-4856).  ``now`` is ``time(0)``, an int in [0, 2^31); ``date`` is ``long_date(1)``, bytes or str of
        0 .. WHO_DATE_LEN bytes without a NUL.  A looker needs only to be a slot: its ``login`` flag picks the header
        (``who`` typed at the name prompt, c:1470), its level and colour are those in the roster.

        The listed users are the slots with a name and ``login == 0``, in ascending slot order, L of them; the looker is
        among them.  Each needs a room with a room record, one in ``[0, look_rooms)``, or no room and an ``away``;
        otherwise the call raises ``ValueError("who: slot N ...")`` before the device is touched.  For looker ``u`` the
        :class:`Who` holds, in order, what these ``write_user`` calls send: ``"\\n~BB*** Current users <date> ***\\n\\n"``
        (without ``~BB`` at the name prompt); a line per listed user ``j`` with ``vis[j] or level[j] <= level[u]``; the
        footer ``"\\nThere are %d visible, %d invisible, 0 remote users.\\nTotal of %d users"`` of L less the invisible, the
        invisible, and L, the same for every looker; ``".\\n\\n"``.  A line is ``"%-*s : %-4s : %-12s : %d mins."`` of
        ``"  <name> <desc>~RS"`` (``*`` first when invisible) padded to ``40 + 3 * colour_com_count`` of it, the level's
        name, the room's name or ``@`` and the ``away`` link's service, and ``(int)(now - last_login) / 60``; then
        ``"~BR(AFK)\\n"`` or ``"\\n"``.  ``colour_com_count`` (c:2563-2583) is not the transducer's count: after a match
        it advances one byte and walks on through the rest of the table, so ``~FBBM`` counts 3.

        One upload (the table, the speaker state, the room table, the descriptions and the login times only after an
        update of theirs; with none, the lookers and the date alone), three kernel launches (WHO_KERNELS, then
        nuts_roster_speak_plan), one download at the bound size and one synchronise, whatever K and the capacity.  A
        call whose variant and bitmap bound exceeds MANY_ARENA_CAP is refused.

        Out of scope: ``.people``, clones and remote users."""
        self._check_open()
        if isinstance(slots, (str, bytes, bytearray)) or not hasattr(slots, "__len__"):
            raise ValueError(f"slots must be a sequence of slots, not {slots!r}")
        if len(slots) == 0:
            raise ValueError("empty call: no lookers")
        if len(slots) * self.capacity >= 2**31 - 1:
            raise ValueError(f"{len(slots)} whos at {self.capacity} slots: K x capacity must be below 2^31 - 1")
        lookers = []
        for k, v in enumerate(slots):
            try:
                lookers.append(self._slot(v))
            except ValueError as e:
                raise ValueError(f"who {k}: {e}") from None
        if not _is_int(now, 0, 2**31 - 1) or isinstance(now, (bool, np.bool_)):
            raise ValueError(f"now must be an int in [0, 2^31), not {now!r}")
        date = _limited_text("date", date, WHO_DATE_LEN)
        listed = np.flatnonzero((self._speech[:, USER_NAME_LEN] != 0) & ((self._flags & ROSTER_FLAGS["login"]) == 0))
        rooms, away = self._room[listed], self._who[listed, 1]
        linked = np.zeros(len(listed), dtype=bool)
        ok = (away >= 0) & (away < self.look_rooms)
        linked[ok] = (self._room_rec[away[ok], 24] & 1) != 0
        bad = np.flatnonzero(~(((rooms >= 0) & (rooms < self.look_rooms)) | ((rooms < 0) & linked)))
        if len(bad):
            j, rm = int(listed[bad[0]]), int(rooms[bad[0]])
            raise ValueError(f"who: slot {j} is in " + (f"room {rm}, which has no room record (look_rooms is {self.look_rooms})"
                             if rm >= 0 else "no room and is not away over a netlink (update(away=))"))
        k, nl = len(lookers), len(listed)
        texts, words = 4 + nl, max(1, (nl + 31) // 32)
        ctext_bytes = _WHO_FIXED_STRIDE + _WHO_ROW * nl
        bound = _variant_at(ctext_bytes, texts) + 4 * k * words
        if bound > MANY_ARENA_CAP:
            raise ValueError(f"call too large: its variant and bitmap bound is {bound} bytes, the cap is {MANY_ARENA_CAP} "
                             f"(MANY_ARENA_CAP): split it")
        lib = _load()
        handle = self._device_handle(lib)
        slot_arr = np.array(lookers, dtype=np.int32)
        dbuf = np.frombuffer(date, dtype=np.uint8) if date else np.zeros(1, dtype=np.uint8)
        clen = np.empty(texts, dtype=np.int32)
        vn, vw = np.empty((texts, 2), dtype=np.int64), np.empty((texts, 2), dtype=np.int32)
        vwsz = np.empty((texts, 2, MAX_WRITES), dtype=np.int32)
        ctext = np.empty(ctext_bytes, dtype=np.uint8)
        var = np.empty(_variant_at(ctext_bytes, texts), dtype=np.uint8)
        line_slot = np.full(max(nl, 1), -1, dtype=np.int32)
        shown = np.zeros((k, words), dtype=np.uint32)
        t = _RosterTiming()
        rc = lib.nd_roster_who(handle, k, _ptr(slot_arr), nl, int(now), _ptr(dbuf), len(date),
                               _ptr(self._table) if self._dirty else None,
                               _ptr(self._speech) if self._speech_dirty or self._private_dirty else None,
                               _ptr(self._rooms) if self._rooms_dirty and self.look_rooms else None,
                               _ptr(self._udesc) if self._udesc_dirty else None,
                               _ptr(self._who) if self._who_dirty else None, _ptr(clen), _ptr(vn), _ptr(vw), _ptr(vwsz),
                               _ptr(ctext), _ptr(var), _ptr(line_slot), _ptr(shown), ctypes.byref(t))
        _check(rc, "device who failed")
        self._dirty = self._speech_dirty = self._private_dirty = self._udesc_dirty = self._who_dirty = False
        if self.look_rooms:
            self._rooms_dirty = False
        tstarts = np.concatenate([np.array(_WHO_FIXED_AT, dtype=np.int64),
                                  _WHO_FIXED_STRIDE + _WHO_ROW * np.arange(nl, dtype=np.int64)])
        return Who(slots=slot_arr, colour=((self._flags[slot_arr] & ROSTER_FLAGS["colour"]) != 0).astype(np.uint8),
                   login=((self._flags[slot_arr] & ROSTER_FLAGS["login"]) != 0).astype(np.uint8),
                   line_slots=line_slot[:nl], shown=shown, texts=ctext, text_starts=tstarts,
                   text_sizes=clen.astype(np.int64), variants=var, variant_starts=_variant_starts(tstarts, clen),
                   variant_sizes=vn, write_counts=vw, write_sizes=vwsz, timing=_timing_of(t))

    def rooms_many(self, slots, *, topics) -> Rooms:
        """What ``rooms(user, show_topics)`` writes for each of ``slots``, K >= 1 lookers (duplicates allowed), in one
        device call (nuts333.c:5661-5700): ``.rmst`` where ``topics`` is True, ``.rmsn`` where it is False.  ``topics`` is a
        bool, or a sequence of one bool per looker.  A looker needs only to be a slot; its colour is the roster's.  The
        roster needs ``look_rooms >= 1``.  Everything malformed raises ``ValueError("rooms N: ...")`` before the device is
        touched.

        For a looker the :class:`Rooms` holds, in order, what these ``write_user`` calls send: the header of its kind
        (c:5672, 5673); a line per listed room in ascending room number; ``"\\n"``.  A room is listed when its record has
        a name: the reference's room list holds no nameless room, as a slot without a name is no user.  The ``.rmst``
        line is ``"%-20s : %9s~RS    %3d    %3d  %s\\n"`` of name, access (``"  ~FGPUB"`` or ``" ~FRPRIV"``, its first byte
        ``*`` when the access is fixed), the users in the room, ``mesg_cnt`` and the topic; the ``.rmsn`` line is
        ``"%-20s : %9s~RS    %3d    %3d     %s   %s~RS  %s\\n"``, ending in `` NO`` or ``YES`` by ``inlink``, the link's
        state (``"   -"`` with neither netlink nor inlink, ``"~FRDOWN"`` with an inlink alone or an unconnected netlink,
        ``"  ~FGUP"``, ``" ~FYVER"``) and the netlink's service, whatever its state.

        The users in room r are the slots with a name, ``login == 0`` and ``room == r``: :meth:`who_many`'s population.
        The reference counts every non-clone user object whose ``room`` is the room (c:5679-5680), and a non-clone user
        has a room only once ``login`` is 0, because ``connect_user`` sets both within one call (c:1745-1758).  Clone
        records are not slots and are not counted; invisible users are.  A slot without a room, or in a room at or past
        ``look_rooms``, is counted nowhere.

        One upload (the table, the speaker state and the room table only after an update of theirs; with none, the
        lookers alone), three kernel launches (ROOMS_KERNELS, then nuts_roster_speak_plan), one download at the bound
        size and one synchronise, whatever K and the capacity.  A call whose variant and count bound exceeds
        MANY_ARENA_CAP is refused.

        Out of scope: ``.people``, ``.netstat`` and the clone listings."""
        self._check_open()
        if isinstance(slots, (str, bytes, bytearray)) or not hasattr(slots, "__len__"):
            raise ValueError(f"slots must be a sequence of slots, not {slots!r}")
        if len(slots) == 0:
            raise ValueError("empty call: no lookers")
        if self.look_rooms < 1:
            raise ValueError("the roster has no room records (look_rooms is 0): there is no room to list")
        lookers = []
        for k, v in enumerate(slots):
            try:
                lookers.append(self._slot(v))
            except ValueError as e:
                raise ValueError(f"rooms {k}: {e}") from None

        def kind(v):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"topics must be a bool, True for .rmst and False for .rmsn, not {v!r}")
            return bool(v)

        if isinstance(topics, (bool, np.bool_)):
            kinds = [kind(topics)] * len(lookers)
        elif _is_text(topics) or not hasattr(topics, "__len__"):
            raise ValueError(f"topics must be a bool or a sequence of one per looker, not {topics!r}")
        elif len(topics) != len(lookers):
            raise ValueError(f"topics: {len(topics)} values for {len(lookers)} lookers")
        else:
            kinds = []
            for k, v in enumerate(topics):
                try:
                    kinds.append(kind(v))
                except ValueError as e:
                    raise ValueError(f"rooms {k}: {e}") from None
        k, nr = len(lookers), self.look_rooms
        texts = 3 + 2 * nr
        ctext_bytes = _ROOMS_FIXED_STRIDE + (_RMST_ROW + _RMSN_ROW) * nr
        bound = _variant_at(ctext_bytes, texts) + 4 * nr
        if bound > MANY_ARENA_CAP:
            raise ValueError(f"call too large: its variant and count bound is {bound} bytes, the cap is {MANY_ARENA_CAP} "
                             f"(MANY_ARENA_CAP): split it")
        lib = _load()
        handle = self._device_handle(lib)
        slot_arr = np.array(lookers, dtype=np.int32)
        kind_arr = np.array(kinds, dtype=np.uint8)
        asked = (1 if kind_arr.any() else 0) | (2 if not kind_arr.all() else 0)
        clen = np.empty(texts, dtype=np.int32)
        vn, vw = np.empty((texts, 2), dtype=np.int64), np.empty((texts, 2), dtype=np.int32)
        vwsz = np.empty((texts, 2, MAX_WRITES), dtype=np.int32)
        ctext = np.empty(ctext_bytes, dtype=np.uint8)
        var = np.empty(_variant_at(ctext_bytes, texts), dtype=np.uint8)
        counts = np.zeros(nr, dtype=np.int32)
        t = _RosterTiming()
        rc = lib.nd_roster_rooms(handle, k, _ptr(slot_arr), asked, _ptr(self._table) if self._dirty else None,
                                 _ptr(self._speech) if self._speech_dirty else None,
                                 _ptr(self._rooms) if self._rooms_dirty else None, _ptr(clen), _ptr(vn), _ptr(vw), _ptr(vwsz),
                                 _ptr(ctext), _ptr(var), _ptr(counts), ctypes.byref(t))
        _check(rc, "device rooms failed")
        self._private_dirty &= not self._speech_dirty         # the whole speaker mirror went up, or none of it
        self._dirty = self._speech_dirty = self._rooms_dirty = False
        tstarts = np.concatenate([np.array(_ROOMS_FIXED_AT, dtype=np.int64),
                                  _ROOMS_FIXED_STRIDE + _RMST_ROW * np.arange(nr, dtype=np.int64),
                                  _ROOMS_FIXED_STRIDE + _RMST_ROW * nr + _RMSN_ROW * np.arange(nr, dtype=np.int64)])
        return Rooms(slots=slot_arr, colour=((self._flags[slot_arr] & ROSTER_FLAGS["colour"]) != 0).astype(np.uint8),
                     topics=kind_arr, counts=counts, texts=ctext, text_starts=tstarts, text_sizes=clen.astype(np.int64),
                     variants=var, variant_starts=_variant_starts(tstarts, clen), variant_sizes=vn, write_counts=vw,
                     write_sizes=vwsz, timing=_timing_of(t))

    @staticmethod
    def _check_sequence(events) -> None:
        """An event call takes a non-empty sequence: what every _prepare_* checks first, before its own settings."""
        if isinstance(events, (str, bytes, bytearray, np.ndarray)) or not hasattr(events, "__len__"):
            raise ValueError(f"events must be a sequence of tuples, not {type(events).__name__}")
        if len(events) == 0:
            raise ValueError("empty call: no events")

    def _prepare_events(self, events, *, actor, rows, texts, coms=None, com_rule=None, need_room_record=True,
                        check_last=(None, None), said=False, then=None):
        """The events of an event call and their actors' state checked, packed for the library: the list of inpstr, their
        offsets and lengths, the slots, the commands and the word counts.  ``coms`` is None for go_many's events, (slot,
        inpstr, word_count); else the events are (slot, com, inpstr, word_count) with com one of ``coms``, and
        ``com_rule`` is how the call says so.  ``actor`` is the call's noun for the slot of an event; rows and texts are
        the call's text rows and its number of texts per event.  ``said`` is clone's: four admit cells an event against
        K x capacity, and a said line in the variant bound, which is then known only behind the loop and checked there.
        check_last is (com, check): check(slot) is the call's own last condition on the events of that command;
        then(coms) is its condition on all of them."""
        n, cells = len(events), "4 x K" if said else "K"
        if (4 if said else 1) * n * self.capacity >= 2**31 - 1:
            raise ValueError(f"{n} events to {self.capacity} slots: {cells} x capacity must be below 2^31 - 1")

        def check_bound(text_bytes):
            bound = _variant_at(sum(rows) * n + text_bytes, texts * n)
            if bound > MANY_ARENA_CAP:
                raise ValueError(f"call too large: its variant bound is {bound} bytes, the cap is {MANY_ARENA_CAP} "
                                 f"(MANY_ARENA_CAP): split it")
        if not said:
            check_bound(0)
        arity, names = (3, "(slot, inpstr, word_count)") if coms is None else (4, "(slot, com, inpstr, word_count)")
        last_com, last_check = check_last
        look_rooms, login, com = self.look_rooms, ROSTER_FLAGS["login"], None
        inps, slots, given, wcs = [], [], [], []
        for k, ev in enumerate(events):
            if not isinstance(ev, tuple) or len(ev) != arity:
                raise ValueError(f"event {k}: expected a {names} tuple, "
                                 f"got {type(ev).__name__}{f' of {len(ev)}' if isinstance(ev, tuple) else ''}")
            try:
                if coms is None:
                    slot, inpstr, wc = ev
                    slot = self._slot(slot)
                else:
                    slot, com, inpstr, wc = ev
                    slot = self._slot(slot)
                    if not _is_int(com, 0, NUM_COMMANDS - 1) or int(com) not in coms:
                        raise ValueError(f"{com_rule}, not {com!r}")
                    given.append(int(com))
                text = _as_text(inpstr)
                if len(text) >= ARR_SIZE:
                    raise ValueError(f"inpstr of {len(text)} bytes: the talker's input line holds at most {ARR_SIZE - 1}")
                if not _is_int(wc, 0, MAX_WORDS):
                    raise ValueError(f"word_count must be an int in [0, {MAX_WORDS}], not {wc!r}")
                room = self._room[slot]
                if need_room_record:
                    if not 0 <= room < look_rooms:
                        raise ValueError(f"the {actor}, slot {slot}, is in " + (f"room {int(room)}, which has no room record"
                                         if room >= 0 else "no room") + f" (look_rooms is {look_rooms})")
                elif room < 0:
                    raise ValueError(f"the {actor}, slot {slot}, is in no room")
                if self._flags[slot] & login:
                    raise ValueError(f"the {actor}, slot {slot}, is still logging in")
                if self._speech[slot, USER_NAME_LEN] == 0:
                    raise ValueError(f"the {actor}, slot {slot}, has no name")
                if last_check is not None and com == last_com:
                    last_check(slot)
            except ValueError as e:
                raise ValueError(f"event {k}: {e}") from None
            inps.append(text)
            slots.append(slot)
            wcs.append(int(wc))
        if then is not None:
            then(given)
        lens = np.fromiter((len(t) for t in inps), dtype=np.int64, count=n)
        if int(lens.sum()) >= 2**31 // 32:
            raise ValueError("call text larger than 64 MiB: split it")
        if said:
            check_bound(_composed_at(int(lens.sum()), n))
        return (inps, _offsets(lens, np.int32), lens.astype(np.int32), np.array(slots, dtype=np.int32),
                np.array(given, dtype=np.uint8), np.array(wcs, dtype=np.uint8))

    def _event_arrays(self, k: int, rows, texts: int, said_bytes: int = 0):
        """The arrays an event call's library function fills in for k events of ``texts`` texts each, ``rows`` bytes an
        event for the fixed ones and said_bytes in all for clone's said lines, as _event_plans takes them: outcome, clen,
        bits (zeroed: the rows addressed to a single slot are set by the binding), vn, vw, vwsz, ctext, var."""
        ctext_bytes = sum(rows) * k + said_bytes
        return (np.empty(k, dtype=np.int8), np.empty((texts, k), dtype=np.int32),
                np.zeros((texts, k, (self.capacity + 63) // 64), dtype=np.uint64), np.empty((texts, k, 2), dtype=np.int64),
                np.empty((texts, k, 2), dtype=np.int32), np.empty((texts, k, 2, MAX_WRITES), dtype=np.int32),
                np.empty(ctext_bytes, dtype=np.uint8), np.empty(_variant_at(ctext_bytes, texts * k), dtype=np.uint8))

    def _event_plans(self, rows, clen, bits, vn, vw, vwsz, var, t, single, said=None):
        """What an event call's library function filled in, as (text_starts, plans, timing): one Plan per text.
        ``single`` lists (text, slots) for the texts that go to one slot alone -- write_user(u, text): ignall, afk and the
        room play no part --, whose bits are set here.  ``said`` is (text, text_off, text_bytes) when that text is
        clone's said line, laid as speak_many lays its own between the fixed rows around it."""
        k = clen.shape[1]
        rows, at = np.array(rows, dtype=np.int64), np.arange(k, dtype=np.int64)
        tstarts = ((np.cumsum(rows) - rows) * k)[:, None] + rows[:, None] * at
        if said is not None:
            row, text_off, text_bytes = said
            tstarts[row:] += _composed_at(text_bytes, k)
            lines = int(rows[:row].sum()) * k + _composed_at(text_off.astype(np.int64), at)
            tstarts = np.concatenate([tstarts[:row], lines[None], tstarts[row:]])
        starts = _variant_starts(tstarts, clen)
        for row, slots in single:
            has = np.flatnonzero(clen[row] >= 0)
            bits[row, has, slots[has] // 64] = np.uint64(1) << (slots[has] % 64).astype(np.uint64)
        timing = _timing_of(t)
        colour_bits = _pack((self._flags & ROSTER_FLAGS["colour"]) != 0)
        plans = [Plan(capacity=self.capacity, admitted_bits=bits[i], colour_bits=colour_bits, variants=var,
                      variant_starts=starts[i], variant_sizes=vn[i], write_counts=vw[i], write_sizes=vwsz[i],
                      timing=dict(timing)) for i in range(len(clen))]
        return tstarts, plans, timing

    def _returned_to_public(self, rm: int) -> None:
        """A room that returned to public, on the host mirrors: access PUBLIC, every slot's invite into it cleared, and its
        review ring emptied when it has one (reset_access, nuts333.c:4605-4611)."""
        self.set_rooms(rm, access=PUBLIC)
        invited = np.flatnonzero(self._go_invite == rm)
        if len(invited):
            self.update(invited, invite_room=None)
        if rm < self.review_rooms:
            self.clear_review([rm])

    def _prepare_go(self, events, gatecrash_level, min_private_users):
        """Each (slot, inpstr, word_count) and its mover's state checked, packed for nd_roster_go: the inpstr, their offsets
        and lengths, the slots and the word counts."""
        self._check_sequence(events)
        if not _is_int(gatecrash_level, 0, MAX_LEVEL):
            raise ValueError(f"gatecrash_level must be an int in [0, {MAX_LEVEL}] (enum np_level), not {gatecrash_level!r}")
        if not _is_int(min_private_users, 0, 2**31 - 1):
            raise ValueError(f"min_private_users must be an int in [0, 2^31), not {min_private_users!r}")
        if self.look_rooms < 1:
            raise ValueError("the roster has no room records (look_rooms is 0): there is no room to go to")
        inps, text_off, lens, slots, _, wcs = self._prepare_events(events, actor="mover", rows=_GO_ROWS, texts=4)
        return b"".join(inps), text_off, lens, slots, wcs

    def go_many(self, events, *, gatecrash_level, min_private_users) -> Go:
        """K ``.go`` events, decided and composed on the device: a non-empty sequence of ``(slot, inpstr, word_count)``
        tuples, what a COMMAND read of :meth:`input_many` with ``com == COM_GO`` hands back -- ``"lounge"`` for ``.go
        lounge`` (nuts333.c:4305-4459).  ``gatecrash_level`` is an int in [0, MAX_LEVEL] and ``min_private_users`` an int >=
        0, the talker's two settings.  The roster needs ``look_rooms >= 1``; every mover needs a room in ``[0, look_rooms)``,
        a name and no ``login`` flag; a slot may appear more than once.  Anything else raises ``ValueError("event k: ...")``
        before the device is touched, and a call whose variant bound exceeds MANY_ARENA_CAP is refused.

        The device does, per event and in the reference's order: ``word[1]`` is the first word of ``inpstr`` as
        ``np_wordfind`` finds it, as :meth:`tell_many` takes its own, not capitalised.  GO_WHERE if ``word_count < 2``;
        GO_NETLINK if the mover's room has a netlink, whatever its state, whose service begins with the word -- nothing is
        composed, the caller does what ``go()`` does over the link; ``get_room`` is the lowest look room with a name that
        begins with the word (a room without a name is no room), else GO_NO_ROOM; GO_ALREADY; GO_NOT_ADJOINED if the room is
        not among the links of the mover's and its level is below WIZ; GO_PRIVATE if ``access & PRIVATE``, the level is
        below ``gatecrash_level``, ``invite_room`` is another room and the room is not a fixed one entered by a WIZ; else
        the move: GO_UNSEEN for an invisible mover, GO_WALKED by a link, GO_TELEPORTED without one.  A move composes the
        enter line for the target room and the leave line for the old room without the mover -- ``invisenter`` and
        ``invisleave``, the two lines of blue magic, or ``"<name> <in_phrase>.\\n"`` and ``"<name> <out_phrase> to the
        <room>.\\n"``.  When the old room's access is exactly PRIVATE and fewer than ``min_private_users`` stay behind --
        the slots with that room, a name and no ``login`` flag, and the clone records standing there -- it returns to
        public: ``"Room access returned to ~FGPUBLIC.\\n"`` to the old room.

        Every event is decided and planned against the roster as it was before the call.  To keep that exact, an event
        whose slot, current room or resolved target room was touched by an earlier event of the call that moved is
        GO_DEFERRED: it wrote nothing and changed nothing, and the caller submits it again in its next call.  A move
        touches its slot, the room left and the room entered; nothing else touches anything.  The events that remain are
        pairwise disjoint in slots and rooms, so each one decided against the snapshot is what running them one after
        another gives.  A call of one event never defers.

        The binding then applies the result to the host mirrors, through :meth:`update`, :meth:`set_rooms` and
        :meth:`clear_review`, in ``move_user``'s order: the movers' rooms, their invites into their targets cleared; if
        anyone moved, one :meth:`look_many` over the movers in event order; then every room that returned to public made
        PUBLIC, with every slot's invite into it cleared and its review ring emptied when it has one.  ``move_user`` looks
        before ``reset_access`` runs (nuts333.c:4457-4458), so a mover's look shows the room it left as it was, and the
        rooms that earlier events returned to public as public.  The one look shows no room of the call as returned, so
        the binding defers one more kind of event: a move whose new room adjoins a room that an earlier event of the
        same call returned to public.  No kernel writes a kept table.  Returns a :class:`Go`.

        A call therefore visits the device at most twice.  The first visit is one upload (the table, the speaker state, the
        clone records, the room table and the go mirror only after an update of theirs), three kernel launches (GO_KERNELS,
        then nuts_roster_speak_plan), one download at the bound size and one synchronise, whatever K and the capacity; the
        second is ``look_many``'s.  After a move the table is stale on the device: the next call of any kind that reads it,
        the look included, uploads its ``5 x capacity`` bytes; a room that returned to public costs the room table and
        the go mirror as well.

        Out of scope: ``.move`` (teleport 2), which is :meth:`act_many`'s; the netlink branch and the ``remote_com == GO`` release, which the caller does
        before it submits; remote users; ``.private``, ``.public``, ``.invite`` and ``.letmein`` themselves -- they are
        :meth:`access_many`'s, which keeps ``access`` and ``invite_room`` for this call; the prompt; fusing the look into the
        first device visit;
        applying the moves by a kernel.  ``go_many`` does not relay to clones' owners; the clone records it counts are
        :meth:`set_clones`' and :meth:`clone_many`'s."""
        self._check_open()
        text, text_off, lens, slots, wcs = self._prepare_go(events, gatecrash_level, min_private_users)
        lib = _load()
        handle = self._device_handle(lib)
        k = len(lens)
        outcome, clen, bits, vn, vw, vwsz, ctext, var = self._event_arrays(k, _GO_ROWS, 4)
        target, old, returned = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int32), np.empty(k, dtype=np.uint8)
        tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        t = _RosterTiming()
        rc = lib.nd_roster_go(handle, k, _ptr(tbuf), len(text), _ptr(text_off), _ptr(lens), _ptr(slots), _ptr(wcs),
                              int(gatecrash_level), int(min_private_users), _ptr(self._table) if self._dirty else None,
                              _ptr(self._speech) if self._speech_dirty else None,
                              _ptr(self._clones) if self._clones_dirty and self.clones else None,
                              _ptr(self._rooms) if self._rooms_dirty else None, _ptr(self._go) if self._go_dirty else None,
                              _ptr(outcome), _ptr(target), _ptr(old), _ptr(returned), _ptr(clen), _ptr(bits), _ptr(vn),
                              _ptr(vw), _ptr(vwsz), _ptr(ctext), _ptr(var), ctypes.byref(t))
        _check(rc, "device go failed")
        self._private_dirty &= not self._speech_dirty         # the whole speaker mirror went up, or none of it
        self._dirty = self._speech_dirty = self._rooms_dirty = self._go_dirty = False
        if self.clones:
            self._clones_dirty = False
        # the device's three, then the mover alone
        tstarts, plans, timing = self._event_plans(_GO_ROWS, clen, bits, vn, vw, vwsz, var, t, [(GO_REPLY, slots)])
        go = Go(outcome=outcome, target=target, old_room=old, returned_public=returned.astype(bool), enter=plans[GO_ENTER],
                leave=plans[GO_LEAVE], reset=plans[GO_RESET], reply=plans[GO_REPLY], texts=ctext, text_starts=tstarts,
                text_sizes=clen.astype(np.int64), look_index=np.full(k, -1, dtype=np.int32), timing=timing)
        # move_user looks before reset_access runs (c:4457-4458): a look shows the rooms that earlier events returned to
        # public as public and the mover's own old room as it was.  One look_many before the resets shows none of them
        # public, so a mover whose new room adjoins a room that an earlier event of the call returned is deferred here
        public = set()
        for k in go.moved().tolist():
            rec = self._room_rec[target[k]]
            if public & set(rec[32:32 + 4 * int(rec[22])].view("<i4").tolist()):
                outcome[k], go.returned_public[k] = GO_DEFERRED, False
                go.text_sizes[:, k] = -1
                for plan in plans:
                    plan.admitted_bits[k], plan.variant_sizes[k], plan.write_counts[k] = 0, 0, 0
            elif go.returned_public[k]:
                public.add(int(old[k]))
        # the moves, on the host mirrors: the next call of any kind uploads what it reads
        moved = go.moved()
        if len(moved):
            movers, into = slots[moved], target[moved]
            self.update(movers, room=into)
            invited = movers[self._go_invite[movers] == into]
            if len(invited):
                self.update(invited, invite_room=None)
            go.look = self.look_many(movers)
            go.look_index[moved] = np.arange(len(moved), dtype=np.int32)
        for rm in sorted(public):
            self._returned_to_public(rm)
        return go

    def _prepare_access(self, events, gatecrash_level, min_private_users, ignore_mp_level):
        """Each (slot, com, inpstr, word_count) and its actor's state checked, packed for nd_roster_access: the inpstr, their
        offsets and lengths, the slots, the commands and the word counts."""
        self._check_sequence(events)
        if not _is_int(gatecrash_level, 0, MAX_LEVEL):
            raise ValueError(f"gatecrash_level must be an int in [0, {MAX_LEVEL}] (enum np_level), not {gatecrash_level!r}")
        if not _is_int(min_private_users, 0, 2**31 - 1):
            raise ValueError(f"min_private_users must be an int in [0, 2^31), not {min_private_users!r}")
        if not _is_int(ignore_mp_level, 0, MAX_LEVEL + 1):
            raise ValueError(f"ignore_mp_level must be an int in [0, {MAX_LEVEL + 1}], not {ignore_mp_level!r}")
        if self.look_rooms < 1:
            raise ValueError("the roster has no room records (look_rooms is 0): there is no room to set or to be let into")
        inps, *packed = self._prepare_events(events, actor="actor", rows=_ACCESS_ROWS, texts=4, coms=_ACCESS_COMS,
                                             com_rule=_ACCESS_COM_RULE)
        return (b"".join(inps), *packed)

    def access_many(self, events, *, gatecrash_level, min_private_users, ignore_mp_level) -> Access:
        """K ``.public`` / ``.private`` / ``.letmein`` / ``.invite`` events, decided and composed on the device: a non-empty
        sequence of ``(slot, com, inpstr, word_count)`` tuples, what a COMMAND read of :meth:`input_many` hands back, with
        ``com`` COM_PUBLIC, COM_PRIVATE, COM_LETMEIN or COM_INVITE (``set_room_access``, ``letmein`` and ``invite``,
        nuts333.c:4543-4693).  ``gatecrash_level`` is an int in [0, MAX_LEVEL], ``min_private_users`` an int >= 0 and
        ``ignore_mp_level`` an int in [0, MAX_LEVEL + 1], the talker's three settings.  The roster needs ``look_rooms >= 1``;
        every actor needs a room in ``[0, look_rooms)``, a name and no ``login`` flag; a slot may appear more than once.
        Anything else raises ``ValueError("event k: ...")`` before the device is touched, and a call whose variant bound
        exceeds MANY_ARENA_CAP is refused.

        The device does, per event and in the reference's order, with ``word[1]`` the first word of ``inpstr`` as
        :meth:`go_many` takes it.  ``.public`` and ``.private``: the room is the actor's own when ``word_count < 2``; else
        ACCESS_LOW_LEVEL below ``gatecrash_level``, and ``get_room`` as :meth:`go_many` runs it, else ACCESS_NO_ROOM.  Then
        ACCESS_FIXED if ``access > PRIVATE``; ACCESS_ALREADY_PUBLIC; ACCESS_ALREADY_PRIVATE; ACCESS_TOO_FEW if the room holds
        fewer than ``min_private_users`` -- the slots with that room, a name and no ``login`` flag, the actor among them,
        and the clone records standing there -- and the actor's level is below ``ignore_mp_level``; else ACCESS_SET_PRIVATE
        or ACCESS_SET_PUBLIC: ``reply`` is ``"Room set to ...\\n"``, and the actor's own room gets ``here`` without the
        actor, ``"<name> has set the room to ...\\n"`` with ``invisname`` for an invisible actor, any other room gets
        ``there``, ``"This room has been set to ...\\n"``.  The refusals say "This room" of the actor's own room and "That
        room" of another.  ``.letmein``: ACCESS_LET_WHERE if ``word_count < 2``; ``get_room``, else ACCESS_LET_NO_ROOM;
        ACCESS_LET_ALREADY; ACCESS_LET_NOT_ADJOINED if the room is not among the links of the actor's, whatever its level;
        ACCESS_LET_PUBLIC unless ``access & PRIVATE``; else ACCESS_ASKED: the reply, ``here`` to the actor's room and
        ``there`` to the room asked, both with the asker's own name even when it is invisible.  ``.invite``:
        ACCESS_INVITE_WHO if ``word_count < 2``; ACCESS_INVITE_PUBLIC unless the actor's room has ``access & PRIVATE``;
        ``get_user`` as :meth:`tell_many` runs it over the word with its first byte capitalised, else ACCESS_INVITE_NOBODY;
        ACCESS_INVITE_SELF; ACCESS_INVITE_HERE; ACCESS_INVITE_ALREADY if the user's ``invite_room`` is this room; else
        ACCESS_INVITED: the reply, and ``notice`` to the invited slot alone, ``"<name> has invited you into the
        <room>.\\n"``.  The room lines' ``com_num`` is the event's ``com``.

        Every event is decided and planned against the roster as it was before the call.  To keep that exact, an event is
        ACCESS_DEFERRED when an earlier event of the same call that was not itself deferred touched its actor's room, the
        room its word resolved to or the slot ``get_user`` found: it wrote nothing and changed nothing, and the caller
        submits it again.  ACCESS_SET_PRIVATE and ACCESS_SET_PUBLIC touch the room whose access changes, ACCESS_INVITED
        touches the invited slot; nothing else touches anything, so a repeated actor alone defers nothing, and a call of
        one event never defers.

        The binding then applies the result to the host mirrors in event order, through :meth:`set_rooms`, :meth:`update`
        and :meth:`clear_review`: a room set private gets ``access=PRIVATE``; a room set public gets ``access=PUBLIC``,
        every slot invited into it loses its ``invite_room`` and its review ring, when it has one, is emptied
        (nuts333.c:4605-4611); an invited slot gets the actor's room as ``invite_room``.  No kernel writes a kept table: a
        following :meth:`go_many`, :meth:`look_many` or :meth:`review_many` uploads what changed and sees the new state.

        A call is one upload (the table, the speaker state, the clone records, the room table and the go mirror only
        after an update of theirs), three kernel launches (ACCESS_KERNELS, then nuts_roster_speak_plan), one download at
        the bound size and one synchronise, whatever K and the capacity.  Returns an :class:`Access`.

        Out of scope: ``.topic``; ``.move``, which is :meth:`act_many`'s; the relay of the two room lines to clones' owners -- the caller passes them
        to :meth:`relay_many`, as after :meth:`go_many`; remote users; the prompt."""
        self._check_open()
        text, text_off, lens, slots, coms, wcs = self._prepare_access(events, gatecrash_level, min_private_users, ignore_mp_level)
        lib = _load()
        handle = self._device_handle(lib)
        k = len(lens)
        outcome, clen, bits, vn, vw, vwsz, ctext, var = self._event_arrays(k, _ACCESS_ROWS, 4)
        target_room, target_slot = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int32)
        tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        t = _RosterTiming()
        rc = lib.nd_roster_access(handle, k, _ptr(tbuf), len(text), _ptr(text_off), _ptr(lens), _ptr(slots), _ptr(coms), _ptr(wcs),
                                  int(gatecrash_level), int(min_private_users), int(ignore_mp_level),
                                  _ptr(self._table) if self._dirty else None, _ptr(self._speech) if self._speech_dirty else None,
                                  _ptr(self._clones) if self._clones_dirty and self.clones else None,
                                  _ptr(self._rooms) if self._rooms_dirty else None, _ptr(self._go) if self._go_dirty else None,
                                  _ptr(outcome), _ptr(target_room), _ptr(target_slot), _ptr(clen), _ptr(bits), _ptr(vn), _ptr(vw),
                                  _ptr(vwsz), _ptr(ctext), _ptr(var), ctypes.byref(t))
        _check(rc, "device access failed")
        self._private_dirty &= not self._speech_dirty         # the whole speaker mirror went up, or none of it
        self._dirty = self._speech_dirty = self._rooms_dirty = self._go_dirty = False
        if self.clones:
            self._clones_dirty = False
        # the device's two, then the actor alone and the invited alone
        tstarts, plans, timing = self._event_plans(_ACCESS_ROWS, clen, bits, vn, vw, vwsz, var, t,
                                                   [(ACCESS_REPLY, slots), (ACCESS_NOTICE, target_slot)])
        access = Access(outcome=outcome, target_room=target_room, target_slot=target_slot, reply=plans[ACCESS_REPLY],
                        here=plans[ACCESS_HERE], there=plans[ACCESS_THERE], notice=plans[ACCESS_NOTICE], texts=ctext,
                        text_starts=tstarts, text_sizes=clen.astype(np.int64), timing=timing)
        # the changes, on the host mirrors and in event order: the next call of any kind uploads what it reads
        for k in access.effective().tolist():
            if outcome[k] == ACCESS_INVITED:
                self.update(int(target_slot[k]), invite_room=int(self._room[slots[k]]))
            elif outcome[k] == ACCESS_SET_PRIVATE:
                self.set_rooms(int(target_room[k]), access=PRIVATE)
            else:
                self._returned_to_public(int(target_room[k]))
        return access

    def _prepare_act(self, events, gatecrash_level, min_private_users):
        """Each (slot, com, inpstr, word_count) and its actor's state checked, packed for nd_roster_act: the inpstr, their
        offsets and lengths, the slots, the commands and the word counts."""
        self._check_sequence(events)
        if not _is_int(gatecrash_level, 0, MAX_LEVEL):
            raise ValueError(f"gatecrash_level must be an int in [0, {MAX_LEVEL}] (enum np_level), not {gatecrash_level!r}")
        if not _is_int(min_private_users, 0, 2**31 - 1):
            raise ValueError(f"min_private_users must be an int in [0, 2^31), not {min_private_users!r}")
        if self.look_rooms < 1:
            raise ValueError("the roster has no room records (look_rooms is 0): there is no room to move anyone to")
        inps, *packed = self._prepare_events(events, actor="actor", rows=_ACT_ROWS, texts=6, coms=_ACT_COMS,
                                             com_rule=_ACT_COM_RULE)
        return (b"".join(inps), *packed)

    def act_many(self, events, *, gatecrash_level, min_private_users) -> Act:
        """K ``.move`` / ``.wake`` / ``.muzzle`` / ``.unmuzzle`` events, the commands a user aims at another user, decided and
        composed on the device: a non-empty sequence of ``(slot, com, inpstr, word_count)`` tuples, what a COMMAND read of
        :meth:`input_many` hands back, with ``com`` COM_MOVE, COM_WAKE, COM_MUZZLE or COM_UNMUZZLE (``move``, ``wake``,
        ``muzzle`` and ``unmuzzle``, nuts333.c:4726-4768, 6496-6522, 6571-6703, with ``move_user(u, rm, 2)``, 4409-4459).
        ``gatecrash_level`` is an int in [0, MAX_LEVEL] and ``min_private_users`` an int >= 0, the talker's two settings.
        The roster needs ``look_rooms >= 1``; every actor needs a room in ``[0, look_rooms)``, a name and no ``login`` flag;
        a slot may appear more than once.  Anything else raises ``ValueError("event k: ...")`` before the device is
        touched, and a call whose variant bound exceeds MANY_ARENA_CAP is refused.

        The device does, per event and in the reference's order, with ``word[1]`` and ``word[2]`` the first two words of
        ``inpstr`` as :meth:`clone_many` takes them, and ``get_user`` over ``word[1]`` as :meth:`tell_many` runs it.
        ``.move``: ACT_MOVE_USAGE if ``word_count < 2``; ACT_MOVE_NOBODY; the room is the actor's own when ``word_count <
        3``, else ``get_room`` over ``word[2]`` as :meth:`go_many` runs it, else ACT_MOVE_NO_ROOM; ACT_MOVE_SELF;
        ACT_MOVE_LEVEL if the target's level is not below the actor's; ACT_MOVE_ALREADY; ACT_MOVE_PRIVATE if the *actor*
        has no access to the room -- ``access & PRIVATE``, the actor's level below ``gatecrash_level``, the actor's
        ``invite_room`` another room and the room not a fixed one entered by a WIZ; ACT_MOVE_AWAY if the target stands in
        no look room (the reference's netlink release): nothing is composed; else ACT_MOVED, or ACT_MOVED_UNSEEN for an
        invisible target.  A move composes ``reply``, ``here`` -- ``"~FT~OL<name> chants an ancient spell...\\n"`` with
        ``invisname`` for an invisible actor --, ``enter`` and ``leave`` -- the vortex and the giant hand with the target's
        name, or ``invisenter`` and ``invisleave`` -- and, for a visible target, the giant hand's ``notice``.  When the
        room left is exactly PRIVATE and fewer than ``min_private_users`` stay behind, counted as :meth:`go_many` counts
        them, it returns to public: ``reset`` to that room.  ``.wake``: ACT_WAKE_USAGE; ACT_WAKE_MUZZLED if the actor's
        ``muzzled`` bit is set; ACT_WAKE_NOBODY; ACT_WAKE_SELF; ACT_WAKE_AFK; else ACT_WOKEN: the reply and the wake-up
        call as ``notice``, with ``invisname`` for an invisible actor.  ``.muzzle``: ACT_MUZZLE_USAGE; ACT_MUZZLE_ABSENT if
        ``get_user`` found nobody -- the reference goes to the user file, nothing is composed; ACT_MUZZLE_SELF;
        ACT_MUZZLE_LEVEL; ACT_MUZZLE_ALREADY if the target's muzzle (see :meth:`update`) is not below the actor's level;
        else ACT_MUZZLED.  ``.unmuzzle``: ACT_UNMUZZLE_USAGE; ACT_UNMUZZLE_ABSENT; ACT_UNMUZZLE_SELF; ACT_UNMUZZLE_NOT,
        which writes nothing, as the reference does (nuts333.c:6656-6658); ACT_UNMUZZLE_ABOVE if the muzzle is above the
        actor's level; else ACT_UNMUZZLED.  The room lines' ``com_num`` is the event's ``com``.

        Every event is decided and planned against the roster as it was before the call.  To keep that exact, an event is
        ACT_DEFERRED when an earlier event of the same call that was not itself deferred touched one of its two slots --
        the actor's and the one ``get_user`` found -- or three rooms -- the actor's, the found slot's and the resolved
        one: it wrote nothing and changed nothing, and the caller submits it again.  A move touches the target's slot, the
        room left and the room entered; a muzzle set or removed touches the target's slot; nothing else touches anything,
        and a call of one event never defers.

        The binding then applies the result to the host mirrors, through :meth:`update`, :meth:`set_rooms` and
        :meth:`clear_review`, in ``move_user``'s order and as :meth:`go_many` does: the targets' rooms; their invitations
        into the rooms entered cleared; if anyone moved, one :meth:`look_many` over the moved targets in event order; then
        every room that returned to public made PUBLIC, with every slot's invite into it cleared and its review ring
        emptied when it has one; then ``muzzle_level`` set to the actor's level, or to 0.  As in :meth:`go_many`, the one
        look shows no room of the call as returned, so the binding defers one more kind of event: a move whose new room
        adjoins a room that an earlier event of the same call returned to public.  No kernel writes a kept table.

        A call therefore visits the device at most twice.  The first visit is one upload (the table, the speaker state, the
        clone records, the room table and the go mirror only after an update of theirs; the speaker state after an update
        of ``afk`` or ``igntell`` as well, since a ``.wake`` reads ``afk``), three kernel launches
        (ACT_KERNELS, then nuts_roster_speak_plan), one download at the bound size and one synchronise, whatever K and the
        capacity; the second is ``look_many``'s.  Returns an :class:`Act`.

        Delivery, per client: the events in call order, and of one event the reply, the here line, the notice, the enter
        line, the leave line, the target's look, the reset line.

        What stays with the caller: the two ``*_ABSENT`` branches, which read and write the user file, and
        ACT_MOVE_AWAY, the release of a user over its netlink (nuts333.c:4439-4443); the syslog lines of a muzzle and an unmuzzle; ``prompt(u)`` for the moved user; the relay of the four room lines
        to clones' owners, through :meth:`relay_many`; remote users; the check of the command's level, which
        :meth:`input_many` makes."""
        self._check_open()
        text, text_off, lens, slots, coms, wcs = self._prepare_act(events, gatecrash_level, min_private_users)
        lib = _load()
        handle = self._device_handle(lib)
        k = len(lens)
        outcome, clen, bits, vn, vw, vwsz, ctext, var = self._event_arrays(k, _ACT_ROWS, 6)
        target_slot, target_room, old = (np.empty(k, dtype=np.int32) for _ in range(3))
        returned = np.empty(k, dtype=np.uint8)
        tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        t = _RosterTiming()
        # ``.wake`` reads a target's ``afk`` bit, which marks _private_dirty alone: the speaker mirror travels for it too
        speech_stale = self._speech_dirty or self._private_dirty
        rc = lib.nd_roster_act(handle, k, _ptr(tbuf), len(text), _ptr(text_off), _ptr(lens), _ptr(slots), _ptr(coms), _ptr(wcs),
                               int(gatecrash_level), int(min_private_users), _ptr(self._table) if self._dirty else None,
                               _ptr(self._speech) if speech_stale else None,
                               _ptr(self._clones) if self._clones_dirty and self.clones else None,
                               _ptr(self._rooms) if self._rooms_dirty else None, _ptr(self._go) if self._go_dirty else None,
                               _ptr(outcome), _ptr(target_slot), _ptr(target_room), _ptr(old), _ptr(returned), _ptr(clen),
                               _ptr(bits), _ptr(vn), _ptr(vw), _ptr(vwsz), _ptr(ctext), _ptr(var), ctypes.byref(t))
        _check(rc, "device act failed")
        self._private_dirty = False                           # the whole speaker mirror went up, or nothing of it was stale
        self._dirty = self._speech_dirty = self._rooms_dirty = self._go_dirty = False
        if self.clones:
            self._clones_dirty = False
        # the device's four, then the actor alone and the target alone
        tstarts, plans, timing = self._event_plans(_ACT_ROWS, clen, bits, vn, vw, vwsz, var, t,
                                                   [(ACT_REPLY, slots), (ACT_NOTICE, target_slot)])
        act = Act(outcome=outcome, target_slot=target_slot, target_room=target_room, old_room=old,
                  returned_public=returned.astype(bool), reply=plans[ACT_REPLY], here=plans[ACT_HERE], enter=plans[ACT_ENTER],
                  leave=plans[ACT_LEAVE], reset=plans[ACT_RESET], notice=plans[ACT_NOTICE], texts=ctext, text_starts=tstarts,
                  text_sizes=clen.astype(np.int64), look_index=np.full(k, -1, dtype=np.int32), timing=timing)
        # as in go_many: a moved target whose new room adjoins a room that an earlier event of the call returned to public
        # would look at it before the one look_many shows it public, and is deferred here
        public = set()
        for b in act.moved().tolist():
            rec = self._room_rec[target_room[b]]
            if public & set(rec[32:32 + 4 * int(rec[22])].view("<i4").tolist()):
                outcome[b], act.returned_public[b] = ACT_DEFERRED, False
                act.text_sizes[:, b] = -1
                for plan in plans:
                    plan.admitted_bits[b], plan.variant_sizes[b], plan.write_counts[b] = 0, 0, 0
            elif act.returned_public[b]:
                public.add(int(old[b]))
        # the changes, on the host mirrors: the next call of any kind uploads what it reads
        moved = act.moved()
        if len(moved):
            movers, into = target_slot[moved], target_room[moved]
            self.update(movers, room=into)
            invited = movers[self._go_invite[movers] == into]
            if len(invited):
                self.update(invited, invite_room=None)
            act.look = self.look_many(movers)
            act.look_index[moved] = np.arange(len(moved), dtype=np.int32)
        for rm in sorted(public):
            self._returned_to_public(rm)
        muzzles = np.flatnonzero((outcome == ACT_MUZZLED) | (outcome == ACT_UNMUZZLED))
        if len(muzzles):                # one update: the order kernel leaves a target one such event a call
            levels = np.where(outcome[muzzles] == ACT_MUZZLED, self._speech[slots[muzzles], _LEVEL_BYTE], 0)
            self.update(target_slot[muzzles], muzzle_level=levels.tolist())
        return act

    def _prepare_clone(self, events, max_clones, gatecrash_level, min_private_users, record):
        """Each (slot, com, inpstr, word_count) and its actor's state checked, packed for nd_roster_clone: the inpstr, their
        offsets and lengths, the slots, the commands and the word counts, whether the call records, and the first record
        behind the last occupied one."""
        self._check_sequence(events)
        if not _is_int(max_clones, 0, 2**31 - 1):
            raise ValueError(f"max_clones must be an int in [0, 2^31), not {max_clones!r}")
        if not _is_int(gatecrash_level, 0, MAX_LEVEL):
            raise ValueError(f"gatecrash_level must be an int in [0, {MAX_LEVEL}] (enum np_level), not {gatecrash_level!r}")
        if not _is_int(min_private_users, 0, 2**31 - 1):
            raise ValueError(f"min_private_users must be an int in [0, 2^31), not {min_private_users!r}")
        record = _flag("record", record)
        if self.look_rooms < 1:
            raise ValueError("the roster has no room records (look_rooms is 0): there is no room for a clone to stand in")
        if self.clones < 1:
            raise ValueError("the roster has no clone records (clones is 0)")
        if record and self.review_rooms < self.look_rooms:
            raise ValueError(f"record: a clone may speak in any of the {self.look_rooms} look rooms, and "
                             f"{self._ring_rooms_are()}")
        # create_user() == NULL has no counterpart: every .clone of the call must find a record behind the last occupied one
        owned = np.flatnonzero(self._clone_owner >= 0)
        tail = int(owned[-1]) + 1 if len(owned) else 0

        def check_free(coms):
            if coms.count(COM_CLONE) > self.clones - tail:
                raise ValueError(f"{coms.count(COM_CLONE)} .clone events, and {self.clones - tail} empty clone records behind the "
                                 f"last occupied one, record {tail - 1}, of {self.clones}: split the call, or make a roster with more")
        inps, *packed = self._prepare_events(events, actor="actor", rows=_CLONE_ROWS, texts=6, coms=_CLONE_COMS,
                                             com_rule=_CLONE_COM_RULE, said=True, then=check_free)
        return (b"".join(inps), *packed, record, tail)

    def clone_many(self, events, *, max_clones, gatecrash_level, min_private_users, record=False) -> Clone:
        """K ``.clone`` / ``.destroy`` / ``.csay`` / ``.chear`` events, decided and composed on the device: a non-empty
        sequence of ``(slot, com, inpstr, word_count)`` tuples, what a COMMAND read of :meth:`input_many` hands back, with
        ``com`` COM_CLONE, COM_DESTROY, COM_CSAY or COM_CHEAR (``create_clone``, ``destroy_clone``, ``clone_say`` and
        ``clone_hear``, nuts333.c:7100-7210, 7293-7357).  :meth:`input_many` has held the command to the speaker's level; this
        call checks no level beyond what those functions check.  ``max_clones`` is an int in [0, 2^31), ``gatecrash_level``
        an int in [0, MAX_LEVEL] and ``min_private_users`` an int >= 0, the talker's three settings.  The roster needs
        ``look_rooms >= 1`` and ``clones >= 1``; every actor needs a room in ``[0, look_rooms)``, a name and no ``login``
        flag; a slot may appear more than once.  ``create_user() == NULL`` has no counterpart: a call that holds more
        ``.clone`` events than there are empty records behind the last occupied one is refused -- by the count of such
        events, not by their outcomes, which only the device knows: one that would be refused or deferred counts, and a
        record an earlier ``.destroy`` of the same call frees does not.  Anything malformed raises
        ``ValueError("event k: ...")`` before the device is touched, with no mirror and no dirty flag changed, and a call
        whose variant bound exceeds MANY_ARENA_CAP is refused.

        The device does, per event and in the reference's order, with ``word[1]`` the first word of ``inpstr`` and
        ``word[2]`` the second, as :meth:`go_many` and :meth:`access_many` take theirs.  ``.clone``: the room is the actor's
        own when ``word_count < 2``, else ``get_room``, else CLONE_NO_ROOM; CLONE_PRIVATE when ``has_room_access`` fails -- the
        room has ``access & PRIVATE``, the actor's level is below ``gatecrash_level``, its ``invite_room`` is another room and
        the room is not a fixed one asked by a WIZ or above.  Then, of the actor's records in record order, which is list
        order: CLONE_ALREADY if one stands in the room and ``max_clones < 1`` or fewer than ``max_clones`` of them precede the
        first that does; else CLONE_MAX if ``max_clones >= 1`` and the actor has that many; else CLONE_CREATED
        (``max_clones`` 0 never refuses).  ``reply`` is the "created here" line in the actor's own room, else the "created in
        the <room>" line; ``here`` goes to the actor's room without the actor, with ``invisname`` for an invisible actor;
        ``there`` to the clone's room without the actor, with the real name -- both even when the two rooms are one.
        ``.destroy``: the room as above, else CLONE_DESTROY_NO_ROOM; with ``word_count > 2``, ``get_user`` over ``word[2]``
        as :meth:`tell_many` runs it, first byte capitalised (``get_user`` does that itself, nuts333.c:2367), else
        CLONE_DESTROY_NOBODY, and CLONE_DESTROY_LEVEL if that user's level is not below the actor's -- the actor's own name
        included; the first record of that owner in that room is destroyed, CLONE_DESTROYED, else CLONE_DESTROY_NONE_OWN or
        CLONE_DESTROY_NONE_THEIRS (``"<name> does not have a clone the <room>.\\n"``, as the reference has it).  When the
        room's access is exactly PRIVATE and fewer than ``min_private_users`` remain -- the slots with that room, a name and
        no ``login`` flag, and the other clone records standing there -- it returns to public: ``reset[k]``, and
        ``reset_plan`` to the whole room.  ``reply`` to the actor, ``here`` as above, ``there`` to the whole room of the clone,
        the actor included if it stands there, ``notice`` to the owner alone when that is not the actor.  ``.csay``:
        CLONE_CSAY_MUZZLED; CLONE_CSAY_USAGE if ``word_count < 3``; ``get_room``, else CLONE_CSAY_NO_ROOM; CLONE_CSAY_NONE
        without a clone of the actor's there; else CLONE_SAID: ``said`` is ``"Clone of <name> <verb>s: <rest>\\n"`` to the
        whole room, ``<rest>`` being ``inpstr`` behind its first word and the verb taken from its last byte as
        :meth:`speak_many` takes it, with no swear check and no reply.  ``.chear``: CLONE_CHEAR_USAGE if ``word_count < 3`` or
        ``word[2]`` is not exactly ``all``, ``swears`` or ``nothing``; CLONE_CHEAR_NO_ROOM; CLONE_CHEAR_NONE; else the value
        set, CLONE_HEAR_ALL, CLONE_HEAR_SWEARS or CLONE_HEAR_NOTHING, with a reply.  The room lines' ``com_num`` is the
        event's ``com``.

        Every event is decided and planned against the roster as it was before the call.  To keep that exact, an event is
        CLONE_DEFERRED when an earlier event of the same call that was not itself deferred touched its owner slot -- the
        user ``get_user`` found, else the actor -- or the room its word resolved to: it wrote nothing, changed nothing and
        recorded nothing, and the caller submits it again.  CLONE_CREATED touches the actor and the room, CLONE_DESTROYED
        the owner and the room; nothing else touches anything, and a call of one event never defers.

        ``record=True`` stores every said line in its room's review ring as ``speak_many(record=True)`` stores a say, in
        event order, after the pending ``clear_review``; every look room must then be a ring room.

        The binding then applies the result to the host mirrors, in event order and by the indices of the records as they
        were, through :meth:`set_clones`, :meth:`set_rooms`, :meth:`update` and :meth:`clear_review`: a ``.chear`` sets
        ``hear``; a destroyed record is emptied; a room that returned to public gets ``access=PUBLIC``, every slot invited
        into it loses its ``invite_room`` and its ring is emptied, as after :meth:`go_many`; a created clone gets the next
        empty record behind the last occupied one, with ``hear`` CLONE_HEAR_ALL.  When all are applied it closes the gaps
        the destroyed records left: later records move down, order kept, so record order stays list order and the indices
        behind a destroyed record decrease.  No kernel writes a kept table: a following :meth:`relay_many`,
        :meth:`access_many`, :meth:`go_many` or :meth:`look_many` uploads what changed and sees the new state.

        A call is one upload (the table, the speaker state, the go mirror, the room table and the clone records only after
        an update of theirs), three kernel launches (CLONE_KERNELS, then nuts_roster_speak_plan) -- four in a call that
        records (nuts_roster_record) --, one download at the bound size and one synchronise, whatever K, the capacity and
        the records.  Returns a :class:`Clone`.

        Out of scope: ``.switch``, which moves the user and ends in a look; ``.myclones`` and ``.allclones``, an ordered
        compaction of their own; the relay of the room lines to clones' owners -- the caller passes them to
        :meth:`relay_many`, which sees the records as this call left them, so a new clone relays the two lines of its own
        creation and a destroyed one relays nothing, as in the reference; remote users; the prompt."""
        self._check_open()
        text, text_off, lens, slots, coms, wcs, recording, tail = self._prepare_clone(events, max_clones, gatecrash_level,
                                                                                      min_private_users, record)
        lib = _load()
        handle = self._device_handle(lib)
        k = len(lens)
        outcome, clen, bits, vn, vw, vwsz, ctext, var = self._event_arrays(k, _CLONE_ROWS, 6, _composed_at(len(text), k))
        target_room, target_slot = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int32)
        rec, reset = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.uint8)
        tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        clear = self._pending_clear() if recording else None
        t = _RosterTiming()
        rc = lib.nd_roster_clone(handle, k, _ptr(tbuf), len(text), _ptr(text_off), _ptr(lens), _ptr(slots), _ptr(coms), _ptr(wcs),
                                 int(gatecrash_level), int(min_private_users), int(max_clones), int(recording),
                                 _ptr(self._table) if self._dirty else None, _ptr(self._speech) if self._speech_dirty else None,
                                 _ptr(self._clones) if self._clones_dirty else None,
                                 _ptr(self._rooms) if self._rooms_dirty else None, _ptr(self._go) if self._go_dirty else None,
                                 _ptr(clear) if clear is not None else None, _ptr(outcome), _ptr(target_room), _ptr(target_slot),
                                 _ptr(rec), _ptr(reset), _ptr(clen), _ptr(bits), _ptr(vn), _ptr(vw), _ptr(vwsz), _ptr(ctext),
                                 _ptr(var), ctypes.byref(t))
        _check(rc, "device clone failed")
        self._private_dirty &= not self._speech_dirty         # the whole speaker mirror went up, or none of it
        self._dirty = self._speech_dirty = self._rooms_dirty = self._go_dirty = self._clones_dirty = False
        if recording:
            self._clear_sent()
        # the here, there and reset lines, the said lines as speak_many lays its own, the replies, the notices: the
        # device's four, then the actor alone and the owner alone
        tstarts, plans, timing = self._event_plans(_CLONE_ROWS, clen, bits, vn, vw, vwsz, var, t,
                                                   [(CLONE_REPLY, slots), (CLONE_NOTICE, target_slot)],
                                                   said=(CLONE_SAID_LINE, text_off, len(text)))
        created = np.full(k, -1, dtype=np.int32)
        clone = Clone(outcome=outcome, target_room=target_room, target_slot=target_slot, record=rec, created=created,
                      reset=reset.astype(bool), reply=plans[CLONE_REPLY], here=plans[CLONE_HERE], there=plans[CLONE_THERE],
                      reset_plan=plans[CLONE_RESET], notice=plans[CLONE_NOTICE], said=plans[CLONE_SAID_LINE], texts=ctext,
                      text_starts=tstarts, text_sizes=clen.astype(np.int64), timing=timing)
        # the changes, on the host mirrors, in event order and by the records' indices as they were: the next call of any
        # kind uploads what it reads
        for k in clone.effective().tolist():
            if outcome[k] <= CLONE_HEAR_ALL:
                self.set_clones(int(rec[k]), hear=int(outcome[k]))
            elif outcome[k] == CLONE_CREATED:
                self.set_clones(tail, owner=int(slots[k]), room=int(target_room[k]))
                created[k], tail = tail, tail + 1
            elif outcome[k] == CLONE_DESTROYED:
                self.set_clones(int(rec[k]), owner=None)
                if clone.reset[k]:
                    self._returned_to_public(int(target_room[k]))
        # the gaps the destroyed records left close: later records move down, order kept, as the user list loses a node
        gone = rec[outcome == CLONE_DESTROYED]
        if len(gone):
            kept = np.setdiff1d(np.arange(tail), gone)                 # a record that lay empty before the call keeps its place among them
            moved = np.full(tail, -1, dtype=np.int32)
            moved[kept] = np.arange(len(kept), dtype=np.int32)
            owner, room, hear = self._clone_owner[kept].copy(), self._clone_room[kept].copy(), self._clone_hear[kept].copy()
            self._clone_owner[:tail], self._clone_room[:tail], self._clone_hear[:tail] = -1, -1, CLONE_HEAR_NOTHING
            self._clone_owner[:len(kept)], self._clone_room[:len(kept)], self._clone_hear[:len(kept)] = owner, room, hear
            made = created >= 0
            created[made] = moved[created[made]]
        return clone

    def _prepare_set(self, events):
        """Each (slot, com, inpstr, word_count) and its actor's state checked, packed for nd_roster_set: the inpstr, their
        offsets and lengths, the slots, the commands and the word counts."""
        self._check_sequence(events)

        def check_topic(slot):
            if not self._room[slot] < self.look_rooms:
                raise ValueError(f"a .topic by slot {slot} in room {int(self._room[slot])}, which has no room record "
                                 f"(look_rooms is {self.look_rooms})")
        return self._prepare_events(events, actor="actor", rows=_SET_ROWS, texts=3, coms=SET_COMS, com_rule=_SET_COM_RULE,
                                    need_room_record=False, check_last=(COM_TOPIC, check_topic))

    def set_many(self, events) -> Settings:
        """K events by which a user sets its own state, decided and composed on the device: a non-empty sequence of
        ``(slot, com, inpstr, word_count)`` tuples, what a COMMAND read of :meth:`input_many` hands back, with ``com`` one
        of the fourteen SET_COMS: COM_MODE, COM_IGNALL, COM_PROMPT, COM_DESC, COM_INPHR, COM_OUTPHR, COM_TOPIC, COM_VIS,
        COM_INVIS, COM_CHARECHO, COM_AFK, COM_COLOUR, COM_IGNSHOUT and COM_IGNTELL (``toggle_mode``, ``toggle_ignall``,
        ``toggle_prompt``, ``set_desc``, ``set_iophrase``, ``set_topic``, ``visibility``, ``toggle_charecho``, ``afk``,
        ``toggle_colour``, ``toggle_ignshout`` and ``toggle_igntell``, nuts333.c:4009, 4463-4539, 4697, 6434, 6881, 7409-7507).
        Every actor needs a room, a name and no ``login`` flag; a slot may appear more than once.  A ``.topic`` needs
        ``look_rooms >= 1`` and its actor's room in ``[0, look_rooms)``; the other thirteen need no room records.  Anything
        else raises ``ValueError("event k: ...")`` before the device is touched, and a call whose variant bound exceeds
        MANY_ARENA_CAP is refused.  A rejected call changes nothing.

        The device does, per event and in the reference's branch order, with ``word[1]`` the first word of ``inpstr`` as
        :meth:`go_many` takes it, cut at 39 bytes.  The six toggles have two outcomes each, by the flag before the call;
        only ``.ignall`` has a ``here`` line, ``"<name> is now ignoring everyone.\\n"`` or ``"<name> is listening
        again.\\n"``, with the real name even of an invisible actor.  ``.vis`` / ``.invis``: SET_ALREADY_VISIBLE,
        SET_ALREADY_INVISIBLE, or SET_VISIBLE / SET_INVISIBLE with a ``here`` line that carries the real name.  ``.colour``:
        SET_COLOUR_TEST when the actor has ``command_mode``, ``ignall`` and ``charmode_echo`` all set -- nothing is written
        and nothing changes, the caller sends the twenty lines of COLOUR_TEST --, else SET_COLOUR_OFF or SET_COLOUR_ON,
        whose reply is written with colour on either way (:class:`Settings`: ``reply_colour``).  ``.desc``: SET_DESC_QUERY
        if ``word_count < 2``, which prints the kept ``desc``; SET_DESC_CLONE if ``word[1]`` contains ``(CLONE)``;
        SET_DESC_LONG if ``inpstr`` is longer than USER_DESC_LEN; else SET_DESC_SET.  ``.inphr`` / ``.outphr``:
        SET_PHRASE_LONG if ``inpstr`` is longer than PHRASE_LEN, first; then the query; then the set.  ``.topic``:
        SET_TOPIC_NONE or SET_TOPIC_QUERY if ``word_count < 2``; SET_TOPIC_LONG past TOPIC_LEN; else SET_TOPIC_SET, with a
        reply and a ``here`` line, ``"<name> has set the topic to: <inpstr>\\n"`` with ``invisname`` for an invisible actor.
        ``.afk``: with ``word_count < 2`` no message is looked at; with ``word[1] == "lock"`` exactly the message is
        ``remove_first(inpstr)`` and the outcome SET_AFK_LOCKED; else the message is the whole ``inpstr`` and the outcome
        SET_AFK.  A message longer than AFK_MESG_LEN is SET_AFK_LONG, before anything is written.  A non-empty message
        is stored and answered with ``reply2``, ``"AFK message set.\\n"``; an empty one keeps the old ``afk_mesg``.  A
        visible actor's room gets ``"<name> goes AFK: <mesg>\\n"``, with the message as it stands after the store, or
        ``"<name> goes AFK...\\n"``; an invisible actor's room gets nothing.  The ``here`` lines' ``com_num`` is the event's
        ``com``.

        Every event is decided and planned against the roster as it was before the call.  To keep that exact, event k is
        SET_DEFERRED when an earlier effective event of the call, itself not deferred, had the same actor; or changed
        ``ignall`` or ``colour`` of a slot in k's actor's room, and k has a ``here`` line; or set the topic of k's actor's
        room, and k is a ``.topic``.  A deferred event wrote nothing and changed nothing, and the caller submits it again.
        Queries and refusals touch nothing, and a call of one event never defers.

        The binding then applies the effective events to the host mirrors in event order, through :meth:`update` and
        ``set_rooms(topic=)``: the toggled flag; ``desc``, ``in_phrase``, ``out_phrase`` or the room's ``topic`` from
        ``inpstr``; ``vis``; ``afk=1`` for both AFK outcomes (the roster keeps ``afk`` as a flag) and ``afk_mesg`` when a
        message was set.  No kernel writes a kept table: the next call of any kind uploads what changed and sees it.

        A call is one upload (the table, the speaker state, the AFK messages, the descriptions and the go mirror only
        after an update of theirs; the room table only after one and when the call holds a ``.topic``), three kernel
        launches (SET_KERNELS, then nuts_roster_speak_plan), one download at the bound size and one synchronise, whatever K
        and the capacity.  The speaker state goes up when any of its three dirty flags is set, and all three are cleared.
        Returns a :class:`Settings`.

        Out of scope: the prompt; the return from AFK (nuts333.c:180-203), and the session lock itself, which stay with
        the caller; remote users and "home execution"; the relay of the ``here`` lines to clones' owners -- the caller
        passes them to :meth:`relay_many`, as after :meth:`access_many`, and an ``.ignall``'s with ``ignall={actor: the
        flag as it was}``, because ``toggle_ignall`` flips the flag behind its line and this call has applied the flip; the commands' level check, which
        :meth:`input_many` has already made."""
        self._check_open()
        inps, text_off, lens, slots, coms, wcs = self._prepare_set(events)
        text = b"".join(inps)
        lib = _load()
        handle = self._device_handle(lib)
        k = len(lens)
        outcome, clen, bits, vn, vw, vwsz, ctext, var = self._event_arrays(k, _SET_ROWS, 3)
        tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        speech_dirty = self._speech_dirty or self._private_dirty or self._set_dirty
        rooms_read = bool((coms == COM_TOPIC).any())
        t = _RosterTiming()
        rc = lib.nd_roster_set(handle, k, _ptr(tbuf), len(text), _ptr(text_off), _ptr(lens), _ptr(slots), _ptr(coms), _ptr(wcs),
                               _ptr(self._table) if self._dirty else None, _ptr(self._speech) if speech_dirty else None,
                               _ptr(self._afk) if self._afk_dirty else None, _ptr(self._udesc) if self._udesc_dirty else None,
                               _ptr(self._go) if self._go_dirty else None,
                               _ptr(self._rooms) if rooms_read and self._rooms_dirty else None,
                               _ptr(outcome), _ptr(clen), _ptr(bits), _ptr(vn), _ptr(vw), _ptr(vwsz), _ptr(ctext), _ptr(var),
                               ctypes.byref(t))
        _check(rc, "device set failed")
        self._dirty = self._speech_dirty = self._private_dirty = self._set_dirty = False
        self._afk_dirty = self._udesc_dirty = self._go_dirty = False
        if rooms_read:
            self._rooms_dirty = False
        # the device's, then the actor alone twice
        tstarts, plans, timing = self._event_plans(_SET_ROWS, clen, bits, vn, vw, vwsz, var, t,
                                                   [(SET_REPLY, slots), (SET_REPLY2, slots)])
        reply_colour = ((self._flags[slots] & ROSTER_FLAGS["colour"]) != 0).astype(np.uint8)
        reply_colour[(outcome == SET_COLOUR_ON) | (outcome == SET_COLOUR_OFF)] = 1
        got = Settings(outcome=outcome, reply=plans[SET_REPLY], reply2=plans[SET_REPLY2], here=plans[SET_HERE],
                       reply_colour=reply_colour, texts=ctext, text_starts=tstarts, text_sizes=clen.astype(np.int64), timing=timing)
        # the changes, on the host mirrors and in event order: the next call of any kind uploads what it reads
        toggles = {SET_MODE_COMMAND: ("command_mode", 1), SET_MODE_SPEECH: ("command_mode", 0), SET_IGNALL_ON: ("ignall", 1),
                   SET_IGNALL_OFF: ("ignall", 0), SET_PROMPT_ON: ("prompt", 1), SET_PROMPT_OFF: ("prompt", 0), SET_VISIBLE: ("vis", 1),
                   SET_INVISIBLE: ("vis", 0), SET_CHARECHO_ON: ("charmode_echo", 1), SET_CHARECHO_OFF: ("charmode_echo", 0),
                   SET_COLOUR_ON: ("colour", 1), SET_COLOUR_OFF: ("colour", 0), SET_IGNSHOUT_ON: ("ignshout", 1),
                   SET_IGNSHOUT_OFF: ("ignshout", 0), SET_IGNTELL_ON: ("igntell", 1), SET_IGNTELL_OFF: ("igntell", 0)}
        texts_set = {SET_DESC_SET: "desc", SET_INPHR_SET: "in_phrase", SET_OUTPHR_SET: "out_phrase"}
        for k in got.effective().tolist():
            slot, oc = int(slots[k]), int(outcome[k])
            if oc in toggles:
                self.update(slot, **{toggles[oc][0]: toggles[oc][1]})
            elif oc in texts_set:
                self.update(slot, **{texts_set[oc]: inps[k]})
            elif oc == SET_TOPIC_SET:
                self.set_rooms(int(self._room[slot]), topic=inps[k])
            elif clen[SET_REPLY2, k] >= 0:                              # SET_AFK, SET_AFK_LOCKED: a message was set
                self.update(slot, afk=1, afk_mesg=inps[k] if oc == SET_AFK else _remove_first(inps[k]))
            else:
                self.update(slot, afk=1)
        return got

    def set_clones(self, clones, *, owner=_KEEP, room=_KEEP, hear=_KEEP) -> None:
        """Set fields of the clone records ``clones`` (a record or a sequence of them, each in ``[0, clones)``), by the
        conventions of :meth:`update` and :meth:`set_rooms`: each field given is one value for every record or a sequence
        of one per record, a field not given stays as it is, a record given more than once takes its last values, and
        nothing changes unless the whole call is valid (``ValueError``).  It does not touch the device; only
        :meth:`relay_many` uploads the records, after a change.

        ``owner`` is a slot, or None for an empty record: that record's room and ``hear`` are reset with it, whatever
        else the entry gives.  ``room`` is a room with a room record, one in ``[0, look_rooms)``: the relay needs its name
        from ``set_rooms(name=)``.  ``hear`` is CLONE_HEAR_NOTHING, CLONE_HEAR_SWEARS or CLONE_HEAR_ALL.  A record given
        an owner without a ``hear`` starts at CLONE_HEAR_ALL, as ``create_user`` sets it (nuts333.c:2743)."""
        self._check_open()
        if isinstance(clones, (int, np.integer)):
            clones = [clones]
        if isinstance(clones, (str, bytes, bytearray)) or not hasattr(clones, "__len__"):
            raise ValueError(f"clones must be a clone record or a sequence of them, not {clones!r}")
        idx = [self._clone(v) for v in clones]
        n = len(idx)

        def hear_of(v):
            if not _is_int(v, CLONE_HEAR_NOTHING, CLONE_HEAR_ALL):
                raise ValueError(f"hear must be CLONE_HEAR_NOTHING, CLONE_HEAR_SWEARS or CLONE_HEAR_ALL (0 .. 2), not {v!r}")
            return int(v)

        is_owner = lambda v: v is None or _is_number(v)
        owners = None if owner is _KEEP else _one_or_each("owner", owner, n, lambda v: -1 if v is None else self._slot(v), is_owner)
        rooms = None if room is _KEEP else _one_or_each("room", room, n, self._look_room, _is_number)
        hears = None if hear is _KEEP else _one_or_each("hear", hear, n, hear_of, _is_number)
        for p, c in enumerate(idx):                           # in order: the last value wins
            if owners is not None and owners[p] < 0:
                self._clone_owner[c], self._clone_room[c], self._clone_hear[c] = -1, -1, CLONE_HEAR_NOTHING
                continue
            if owners is not None:
                self._clone_owner[c] = owners[p]
                self._clone_hear[c] = CLONE_HEAR_ALL
            if rooms is not None:
                self._clone_room[c] = rooms[p]
            if hears is not None:
                self._clone_hear[c] = hears[p]
        if n and (owners is not None or rooms is not None or hears is not None):
            self._clones_dirty = True

    def _clone(self, v) -> int:
        if not _is_int(v, 0, self.clones - 1):
            raise ValueError(f"clone record {v!r}: " + (f"the records are 0 .. {self.clones - 1}" if self.clones else
                             "the roster has none (clones is 0)"))
        return int(v)

    def _prepare_relay(self, broadcasts, record, clone_sender):
        """What _prepare_plan returns, the clone senders (-1: none) and the look rooms' names as nd_roster_relay takes
        them, after every check of relay_many."""
        if self.clones == 0:
            raise ValueError("the roster has no clone records (clones is 0): plan_many answers its broadcasts whole")
        packed = self._prepare_plan(broadcasts, record)
        lens, rms, senders = packed[2], packed[3], packed[4]
        k = len(lens)
        if clone_sender is None:
            csender = np.full(k, -1, dtype=np.int32)
        else:
            if isinstance(clone_sender, (str, bytes, bytearray)) or not hasattr(clone_sender, "__len__"):
                raise ValueError(f"clone_sender must be None or a sequence of one clone record or None per broadcast, "
                                 f"not {clone_sender!r}")
            if len(clone_sender) != k:
                raise ValueError(f"clone_sender: {len(clone_sender)} values for {k} broadcasts")
            csender = np.empty(k, dtype=np.int32)
            for b, v in enumerate(clone_sender):
                try:
                    csender[b] = -1 if v is None else self._clone(v)
                except ValueError as e:
                    raise ValueError(f"broadcast {b}: clone_sender: {e}") from None
                if v is not None and senders[b] >= 0:
                    raise ValueError(f"broadcast {b}: its user is clone record {int(v)}, so its sender must be None, "
                                     f"not slot {int(senders[b])}")
        owned = np.flatnonzero(self._clone_owner >= 0)
        for c in owned.tolist():
            if not 0 <= self._clone_owner[c] < self.capacity:
                raise ValueError(f"clone record {c}: its owner, slot {int(self._clone_owner[c])}, is out of range")
            if not 0 <= self._clone_room[c] < self.look_rooms:
                raise ValueError(f"clone record {c}: its room" + (f", {int(self._clone_room[c])}," if self._clone_room[c] >= 0
                                 else "") + f" has no room record (look_rooms is {self.look_rooms}): set_clones(room=)")
        name_len = self._room_rec[:, ROOM_NAME_LEN].astype(np.int64)
        cloned = np.zeros(max(self.look_rooms, 1), dtype=bool)       # the rooms that hold a clone record, whatever its hear
        cloned[self._clone_room[owned]] = True
        for b in range(k):
            rm = int(rms[b])
            if 0 <= rm < self.look_rooms and cloned[rm] and RELAY_EXTRA + int(name_len[rm]) + int(lens[b]) > ARR_SIZE - 1:
                raise ValueError(f"broadcast {b}: room {rm} holds a clone, and the relay text of its {int(lens[b])} bytes "
                                 f"and the room's {int(name_len[rm])}-byte name would be "
                                 f"{RELAY_EXTRA + int(name_len[rm]) + int(lens[b])} bytes: the reference's text2 holds at "
                                 f"most {ARR_SIZE - 1}")
        text_bytes = int(lens.sum(dtype=np.int64))
        bound = _variant_at(text_bytes, k) + _variant_at(_composed_at(text_bytes, k, _RELAY_SLACK), k)
        if bound > MANY_ARENA_CAP:
            raise ValueError(f"call too large: its variant bound over the texts and the relay texts is {bound} bytes, the "
                             f"cap is {MANY_ARENA_CAP} (MANY_ARENA_CAP): split it")
        names = np.zeros((self.look_rooms, _RELAY_NAME_ROW), dtype=np.uint8)
        names[:, :ROOM_NAME_LEN + 1] = self._room_rec[:, :ROOM_NAME_LEN + 1]
        return packed, csender, names

    def _table_with_ignall(self, ignall) -> np.ndarray:
        """A copy of the table mirror with the ``ignall`` flags of ``relay_many(ignall=)``, checked."""
        if not isinstance(ignall, dict) or not ignall:
            raise ValueError(f"ignall must be None or a non-empty dict of slot -> 0/1, not {ignall!r}")
        table = self._table.copy()
        flags = table[4 * self.capacity:]
        for slot, v in ignall.items():
            try:
                j, on = self._slot(slot), _flag("its flag", v)
            except ValueError as e:
                raise ValueError(f"ignall: {e}") from None
            flags[j] = (int(flags[j]) & (0xFF ^ ROSTER_FLAGS["ignall"])) | (ROSTER_FLAGS["ignall"] if on else 0)
        return table

    def relay_many(self, broadcasts, record=None, clone_sender=None, ignall=None) -> Relay:
        """``write_room_except`` whole for K broadcasts to a roster with clone records, in one device call
        (nuts333.c:1401-1429).  ``broadcasts`` and ``record`` are what :meth:`plan_many` takes, checked by the same
        rules; ``clone_sender`` is None, or K entries each None or the clone record that is ``user`` in
        ``write_room_except(rm, str, user)`` (``clone_switch``, nuts333.c:7283) -- that broadcast's ``sender`` must then
        be None.  Returns a :class:`Relay`: its ``plan`` equals ``plan_many(broadcasts, record)`` field by field, and
        the rings end up as after it.

        ``ignall`` is None, or a dict of slot -> 0/1: the whole call, predicate and relay, runs over the roster with these
        slots' ``ignall`` flags as given instead of the roster's.  It is for the one line the reference writes while a
        flag is not yet what an earlier call has made it: ``toggle_ignall`` sends its line and flips the flag last
        (nuts333.c:4466-4476), :meth:`set_many` has applied the flip, so the caller relays the ``here`` line of a
        SET_IGNALL_ON with ``ignall={actor: 0}`` and that of a SET_IGNALL_OFF with ``ignall={actor: 1}`` -- the actor's own
        clone in its room relays "is now ignoring everyone" to it and not "is listening again".  The roster's mirrors do
        not change; such a call uploads its own copy of the table and leaves the table to be uploaded again.

        A clone standing in room ``rm`` does not receive a broadcast, it sends ``"~FT[ <room name> ]:~RS " + text`` to
        its owner.  Clone record ``c`` relays broadcast ``k`` iff ``rm`` is not None and the record has an owner; its
        room equals ``rm``; ``c`` is not ``clone_sender[k]``; its ``hear`` is not CLONE_HEAR_NOTHING; the owner's
        ``ignall`` flag is clear, which ``force_listen`` does not override (nuts333.c:1417); and its ``hear`` is
        CLONE_HEAR_ALL or the text holds a swear word (``np_contains_swearing``).  ``com_num`` plays no part, and a
        clone is never ``login``, ``ignall`` or ``ignshout``.

        Delivery: for broadcast ``k`` a talker writes ``plan.variant(k, colour[j])`` to every admitted slot ``j``, then,
        for every relaying record ``c`` in ascending order, ``relay_variant(k, colour[owner[c]])`` to ``owner[c]``.
        Direct, then relay, is the reference's order per socket, because a clone is always created after its owner
        logged in.

        Rejected with ``ValueError`` before the device is touched, with no mirror changed: a roster without clone
        records; an owned record whose room has no room record or whose owner is no slot; a bad ``clone_sender``; a
        broadcast to a room that holds a clone record, whatever its ``hear``, whose relay text would not fit the
        reference's ``text2[ARR_SIZE]``, ``12 + len(name) + len(text) > ARR_SIZE - 1`` (the reference overflows a stack
        buffer there); and a call whose variant bound over the texts and the relay texts exceeds MANY_ARENA_CAP.

        One upload (the table and the clone records only after an update of theirs, the rooms' names, 24 bytes per look
        room, only when one changed since the last ``relay_many``), three kernel launches (nuts_roster_plan,
        nuts_roster_relay, nuts_roster_speak_plan over the relay texts) -- four in a call that records
        (nuts_roster_record) --, one download at the bound size and one synchronise, whatever K, the capacity and the
        records.

        Out of scope: ``.clone``, ``.destroy``, ``.csay`` and ``.chear`` themselves -- they are :meth:`clone_many`'s, which
        keeps the records for this call --, ``.switch`` -- the caller calls :meth:`set_clones` --, and remote users."""
        self._check_open()
        packed, csender, names = self._prepare_relay(broadcasts, record, clone_sender)
        text, text_off, lens, rm, sender, flags, coms = packed
        table = self._table if ignall is None else self._table_with_ignall(ignall)
        recording = bool((flags & _RECORD_BIT).any())
        new_names = self._relay_names is None or not np.array_equal(names, self._relay_names)
        lib = _load()
        handle = self._device_handle(lib)
        k, words, cwords = len(lens), (self.capacity + 63) // 64, (self.clones + 63) // 64
        rtext_bytes = _composed_at(len(text), k, _RELAY_SLACK)
        bits = np.empty((k, words), dtype=np.uint64)
        vn, rvn = np.empty((k, 2), dtype=np.int64), np.empty((k, 2), dtype=np.int64)
        vw, rvw = np.empty((k, 2), dtype=np.int32), np.empty((k, 2), dtype=np.int32)
        vwsz, rvwsz = np.empty((k, 2, MAX_WRITES), dtype=np.int32), np.empty((k, 2, MAX_WRITES), dtype=np.int32)
        var = np.empty(_variant_at(len(text), k), dtype=np.uint8)
        rbits, rlen = np.empty((k, cwords), dtype=np.uint64), np.empty(k, dtype=np.int32)
        rtext, rvar = np.empty(rtext_bytes, dtype=np.uint8), np.empty(_variant_at(rtext_bytes, k), dtype=np.uint8)
        tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        t = _RosterTiming()
        args = (handle, k, _ptr(tbuf), len(text), _ptr(text_off), _ptr(lens), _ptr(rm), _ptr(sender), _ptr(flags),
                _ptr(coms), _ptr(csender), _ptr(table) if self._dirty or ignall is not None else None,
                _ptr(self._clones) if self._clones_dirty else None, _ptr(names) if new_names else None, _ptr(bits),
                _ptr(vn), _ptr(vw), _ptr(vwsz), _ptr(var), _ptr(rbits), _ptr(rlen), _ptr(rvn), _ptr(rvw), _ptr(rvwsz),
                _ptr(rtext), _ptr(rvar), ctypes.byref(t))
        if recording:                       # the pending clears go first, with the same upload
            clear = self._pending_clear()
            rc = lib.nd_roster_relay_record(*args, _ptr(clear) if clear is not None else None)
        else:
            rc = lib.nd_roster_relay(*args)
        _check(rc, "device relay failed")
        self._dirty, self._clones_dirty = ignall is not None, False     # a table with other flags is on the device
        self._relay_names = names
        if recording:
            self._clear_sent()
        timing = _timing_of(t)
        plan = Plan(capacity=self.capacity, admitted_bits=bits,
                    colour_bits=_pack((self._flags & ROSTER_FLAGS["colour"]) != 0), variants=var,
                    variant_starts=_variant_starts(text_off, lens), variant_sizes=vn, write_counts=vw,
                    write_sizes=vwsz, timing=dict(timing))
        tstarts = _composed_at(text_off.astype(np.int64), np.arange(k, dtype=np.int64), _RELAY_SLACK)
        owner = self._clone_owner.copy()
        colour = np.where(owner >= 0, (self._flags[np.maximum(owner, 0)] & ROSTER_FLAGS["colour"]) != 0, False)
        return Relay(plan=plan, clones=self.clones, relay_bits=rbits, clone_owner=owner,
                     owner_colour=colour.astype(np.uint8), texts=rtext, text_starts=tstarts,
                     text_sizes=rlen.astype(np.int64), variants=rvar, variant_starts=_variant_starts(tstarts, rlen),
                     variant_sizes=rvn, write_counts=rvw, write_sizes=rvwsz, timing=timing)

    def _tell_clear_sent(self) -> None:
        self._tell_clear[:] = 0
        self._tell_clear_pending = False

    def _revtell_slots(self, slots, what: str) -> np.ndarray:
        if not self.revtell:
            raise ValueError("the roster has no revtell rings (revtell is False)")
        if isinstance(slots, (str, bytes, bytearray)) or not hasattr(slots, "__len__"):
            raise ValueError(f"{what} must be a sequence of slots, not {slots!r}")
        return np.array([self._slot(v) for v in slots], dtype=np.int32)

    def clear_revtell(self, slots) -> None:
        """Empty the revtell rings of ``slots``, a slot or a sequence of them, for when a slot changes hands: their lines
        become empty and their cursor 0.  Like :meth:`clear_review` it does not touch the device; it takes effect before
        the records of the next recording :meth:`tell_many` or the next :meth:`revtell_many`, in the order the caller
        issued them."""
        self._check_open()
        idx = self._revtell_slots([slots] if isinstance(slots, (int, np.integer)) else slots, "slots")
        if len(idx):
            self._tell_clear[idx] = 1
            self._tell_clear_pending = True

    def revtell_many(self, slots) -> Review:
        """What ``.revtell`` sends for each of ``slots`` between its header and its footer (nuts333.c:7699-7715), a
        non-empty sequence of slots (duplicates allowed), as a :class:`Review` whose ``rooms`` are the slots, ``stored``
        is ``[Q, 5, 202]`` and whose variants are bounded by MAX_REVTELL_BYTES in MAX_REVTELL_WRITES writes.  One upload,
        one kernel (nuts_roster_revtell), one download, one synchronise.  Anything else raises ``ValueError`` before the
        device is touched."""
        self._check_open()
        idx = self._revtell_slots(slots, "slots")
        q = len(idx)
        if q == 0:
            raise ValueError("empty call: no slots to review")
        if 2 * q * _REVTELL_STRIDE > MANY_ARENA_CAP:
            raise ValueError(f"call too large: {q} slots x 2 x {_REVTELL_STRIDE} bytes exceed the cap of {MANY_ARENA_CAP} "
                             f"(MANY_ARENA_CAP): split it")
        lib = _load()
        clear = self._tell_clear.copy() if self._tell_clear_pending else None
        review = self._review_of(lib.nd_roster_revtell, self._device_handle(lib), idx, clear, REVTELL_LINES)
        self._tell_clear_sent()
        return review

    def _ring_room(self, v) -> int:
        if not _is_int(v, 0, self.review_rooms - 1):
            raise ValueError(f"room {v!r} has no review ring: {self._ring_rooms_are()}")
        return int(v)

    def _ring_rooms(self, rooms, what: str) -> np.ndarray:
        if isinstance(rooms, (str, bytes, bytearray)) or not hasattr(rooms, "__len__"):
            raise ValueError(f"{what} must be a sequence of ring rooms, not {rooms!r}")
        return np.array([self._ring_room(v) for v in rooms], dtype=np.int32)

    def clear_review(self, rooms) -> None:
        """``clear_revbuff`` (as ``.revclr`` uses it) for ``rooms``, a ring room or a sequence of them: their lines
        become empty and their cursor 0.  Like :meth:`update` it does not touch the device; it takes effect before the
        records and reviews of the next recording or reviewing call, in the order the caller issued them."""
        self._check_open()
        idx = self._ring_rooms([rooms] if isinstance(rooms, (int, np.integer)) else rooms, "rooms")
        if len(idx):
            self._clear[idx] = 1
            self._clear_pending = True

    def review_many(self, rooms) -> Review:
        """What ``.review`` sends for each of ``rooms``, a non-empty sequence of ring rooms (duplicates allowed), as a
        :class:`Review`.  One upload, one kernel, one download, one synchronise, whatever the number of rooms and
        whatever the rings hold: every variant is fetched at its bound size, about 40 KB per room.  Anything else raises
        ``ValueError`` before the device is touched."""
        self._check_open()
        idx = self._ring_rooms(rooms, "rooms")
        q = len(idx)
        if q == 0:
            raise ValueError("empty call: no rooms to review")
        if 2 * q * _REVIEW_STRIDE > MANY_ARENA_CAP:
            raise ValueError(f"call too large: {q} rooms x 2 x {_REVIEW_STRIDE} bytes exceed the cap of {MANY_ARENA_CAP} "
                             f"(MANY_ARENA_CAP): split it")
        lib = _load()
        review = self._review_of(lib.nd_roster_review, self._device_handle(lib), idx, self._pending_clear(), REVIEW_LINES)
        self._clear_sent()
        return review

    def _review_of(self, call, handle, idx, clear, lines: int) -> Review:
        """The Review of rings ``idx`` of ``lines`` lines each, through nd_roster_review or nd_roster_revtell."""
        q, stride, writes = len(idx), (lines * MAX_LINE_BYTES + 3) & ~3, lines * MAX_LINE_WRITES
        counts = np.empty(q, dtype=np.int32)
        seq = np.empty(q, dtype=np.int32)
        vn = np.empty((q, 2), dtype=np.int32)
        vw = np.empty((q, 2), dtype=np.int32)
        vwsz = np.empty((q, 2, writes), dtype=np.int32)
        stored = np.empty((q, lines, REVIEW_LEN + 2), dtype=np.uint8)
        var = np.empty(2 * q * stride, dtype=np.uint8)
        t = _RosterTiming()
        rc = call(handle, q, _ptr(idx), _ptr(clear) if clear is not None else None, _ptr(counts), _ptr(seq), _ptr(vn),
                  _ptr(vw), _ptr(vwsz), _ptr(stored), _ptr(var), ctypes.byref(t))
        _check(rc, "device review failed")
        starts = (np.arange(2 * q, dtype=np.int64) * stride).reshape(q, 2)
        return Review(rooms=idx, line_counts=counts, stored=stored, variants=var, variant_starts=starts,
                      variant_sizes=vn.astype(np.int64), write_counts=vw, write_sizes=vwsz, sequential=seq,
                      timing=_timing_of(t))

    def close(self) -> None:
        """Free the device table and the review rings; the roster cannot be used afterwards.  Closing twice is
        harmless."""
        if self._handle is not None and _LIB is not None:
            _LIB.nd_roster_destroy(self._handle)
        self._handle = None
        self._closed = True

    def __enter__(self) -> "Roster":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        if getattr(self, "_handle", None) is not None:
            self.close()
