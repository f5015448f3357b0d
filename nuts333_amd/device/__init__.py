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
COM_SAY, COM_SHOUT, COM_SEMOTE = 3, 4, 7
#: the kernels of fanout.hip, as rocprofv3 names them (the scans are rocPRIM's)
KERNELS = ("nuts_fanout_measure_broadcast", "nuts_fanout_emit_broadcast",
           "nuts_fanout_measure_batch", "nuts_fanout_emit_batch",
           "nuts_fanout_measure_many", "nuts_fanout_emit_many",
           "nuts_roster_measure", "nuts_roster_emit", "nuts_roster_plan")
#: broadcast_many() refuses a call whose arena bound, the sum over its broadcasts of N * max_bytes(len), exceeds this;
#: Roster.plan_many() one whose variant bound, 12 * text bytes + 16 * K, does
MANY_ARENA_CAP = 2 << 30
#: the most slots a Roster holds
MAX_CAPACITY = 65536
#: a room id is None (no room) or an int in [0, ROOM_LIMIT)
ROOM_LIMIT = 2**31 - 1


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


def chunks(result: Fanout, i: int) -> list[bytes]:
    """Item ``i`` as the list of ``write(2)`` chunks the reference would issue."""
    data = result.output(i)
    sizes = result.write_sizes[result.write_offsets[i]:result.write_offsets[i + 1]]
    out, at = [], 0
    for s in sizes.tolist():
        out.append(data[at:at + s])
        at += s
    if at != len(data):
        raise AssertionError(f"item {i}: chunk sizes sum to {at}, arena slot holds {len(data)} bytes")
    return out


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


def _unpack(words: np.ndarray, capacity: int) -> np.ndarray:
    """uint64 [..., W] bitmap words -> bool [..., capacity]: bit j % 64 of word j // 64 is slot j."""
    b = np.ascontiguousarray(words, dtype="<u8").view(np.uint8)
    return np.unpackbits(b, axis=-1, bitorder="little")[..., :capacity].astype(bool)


def _pack(flags: np.ndarray) -> np.ndarray:
    """bool [capacity] -> uint64 [W] bitmap words, the tail bits of the last word zero."""
    padded = np.zeros((len(flags) + 63) // 64 * 64, dtype=bool)
    padded[:len(flags)] = flags
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


@dataclass
class Plan:
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

    def variant(self, k: int, c: int) -> bytes:
        """The bytes broadcast ``k`` sends to a listener with colour bit ``c``."""
        self._check(k, c)
        at = int(self.variant_starts[k, c])
        return self.variants[at:at + int(self.variant_sizes[k, c])].tobytes()

    def chunks(self, k: int, c: int) -> list[bytes]:
        """``variant(k, c)`` as the list of ``write(2)`` chunks the reference would issue."""
        data = self.variant(k, c)
        out, at = [], 0
        for s in self.write_sizes[k, c, :int(self.write_counts[k, c])].tolist():
            out.append(data[at:at + s])
            at += s
        if at != len(data):
            raise AssertionError(f"variant ({k}, {c}): chunk sizes sum to {at}, the variant holds {len(data)} bytes")
        return out

    def expand(self) -> Fanout:
        """The :class:`Fanout` that ``Roster.broadcast_many`` returns for the same call (``timing`` aside), from this
        plan's own arrays alone: item ``(k, j)`` is ``variant(k, colour of j)`` if slot ``j`` is admitted."""
        k, cap = len(self.admitted_bits), self.capacity
        admitted = _unpack(self.admitted_bits, cap).reshape(k * cap)
        colour = _unpack(self.colour_bits, cap).astype(np.intp)
        sizes = np.asarray(self.variant_sizes, dtype=np.int64)[:, colour].reshape(k * cap)
        writes = np.asarray(self.write_counts, dtype=np.int64)[:, colour].reshape(k * cap)
        out_off = np.zeros(k * cap + 1, dtype=np.int64)
        np.cumsum(np.where(admitted, sizes, 0), out=out_off[1:])
        w_off = np.zeros(k * cap + 1, dtype=np.int64)
        np.cumsum(np.where(admitted, writes, 0), out=w_off[1:])
        items = np.flatnonzero(admitted)
        var = 2 * (items // cap) + colour[items % cap]                    # each admitted item's variant, as 2k + c
        arena = _gather(np.asarray(self.variants, dtype=np.uint8),
                        np.asarray(self.variant_starts, dtype=np.int64).reshape(2 * k)[var], sizes[items])
        wsz = _gather(np.asarray(self.write_sizes, dtype=np.int32).reshape(2 * k * MAX_WRITES), var * MAX_WRITES,
                      writes[items])
        return Fanout(admitted=admitted, out_offsets=out_off, arena=arena, write_offsets=w_off, write_sizes=wsz,
                      timing=dict(self.timing), broadcast_offsets=np.arange(k + 1, dtype=np.int64) * cap)


# ------------------------------------------------------------------ validation (never touches the device)
def _as_text(t) -> bytes:
    if isinstance(t, str):
        try:
            t = t.encode("latin-1")
        except UnicodeEncodeError as e:
            raise ValueError(f"text has a character outside one byte: {e}") from None
    elif isinstance(t, (bytearray, memoryview)):
        t = bytes(t)
    if not isinstance(t, bytes):
        raise ValueError(f"text must be bytes or str, not {type(t).__name__}")
    if b"\0" in t:
        raise ValueError("text contains a NUL byte (the talker's strings end there)")
    if len(t) >= TEXT_SIZE:
        raise ValueError(f"text of {len(t)} bytes: the talker's text buffer holds at most {TEXT_SIZE - 1}")
    return t


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
    offs = np.zeros(len(texts), dtype=np.int32)
    np.cumsum(lens[:-1], out=offs[1:])
    return b"".join(texts), offs, lens, rec


def _prepare_broadcast(text, listeners, rm_is_null, force_listen, com_num):
    text = _as_text(text)
    rec = _listener_records(listeners)
    flags = _flag("rm_is_null", rm_is_null), _flag("force_listen", force_listen)
    return text, rec, flags[0], flags[1], _com_num(com_num)


def _com_num(v) -> int:
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) < NUM_COMMANDS:
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
    item_off = np.zeros(len(texts) + 1, dtype=np.int32)
    np.cumsum(ns, out=item_off[1:])
    text_off = np.zeros(len(texts), dtype=np.int32)
    np.cumsum(lens[:-1], out=text_off[1:])
    return (b"".join(texts), text_off, lens.astype(np.int32), np.array(flags, dtype=np.uint8),
            np.array(coms, dtype=np.int32), item_off, np.concatenate(recs))


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
        lib.nd_arena.restype = P
        lib.nd_write_sizes.restype = P
        _LIB = lib
    return _LIB


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
    if rc != 0:
        raise RuntimeError(f"device fan-out failed: {lib.nd_last_error().decode(errors='replace')}")
    return _result(lib, admitted, out_off, w_off, t)


def _result(lib, admitted, out_off, w_off, t: _Timing) -> Fanout:
    """The Fanout of the last call: the arena and the chunk sizes copied out of the library's pinned buffers."""
    nbytes, nwrites = int(out_off[-1]), int(w_off[-1])
    arena = np.ctypeslib.as_array(ctypes.cast(lib.nd_arena(), ctypes.POINTER(ctypes.c_uint8)), (max(nbytes, 1),))
    wsz = np.ctypeslib.as_array(ctypes.cast(lib.nd_write_sizes(), ctypes.POINTER(ctypes.c_int32)), (max(nwrites, 1),))
    return Fanout(admitted=admitted.astype(bool), out_offsets=out_off, arena=arena[:nbytes].copy(),
                  write_offsets=w_off.astype(np.int64), write_sizes=wsz[:nwrites].copy(),
                  timing={"kernels_us": t.kernels_us, "end_to_end_us": t.end_to_end_us})


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
    if rc != 0:
        raise RuntimeError(f"device fan-out failed: {lib.nd_last_error().decode(errors='replace')}")
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
    if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)) or not 0 <= int(v) < ROOM_LIMIT:
        raise ValueError(f"room must be None or an int in [0, {ROOM_LIMIT}), not {v!r}")
    return int(v)


class Roster:
    """The talker's user list, kept on the device between calls: per slot a room (``None``: an empty slot, or a user
    away over a netlink) and the ``login``, ``ignall``, ``ignshout`` and ``colour`` flags.  Broadcasts are addressed as
    ``write_room_except(rm, str, user)`` addresses them (nuts333.c:1401-1415): ``rm`` is a room or ``None`` for every
    room, ``sender`` a slot or ``None``.  The device builds each listener's record from its slot and the broadcast, so a
    call carries K texts and K small tuples; the table travels only in the first call after an :meth:`update`.
    :meth:`broadcast_many` returns every slot's bytes in an arena (a :class:`Fanout`), :meth:`plan_many` the two variants
    and an admit bitmap per broadcast (a :class:`Plan`); they may be mixed in any order.

    Building and updating a roster does not touch the device; its first call allocates there.  The
    contract, for every call::

        roster.broadcast_many(bs) == broadcast_many([(t, roster.table(rm, s), rm is None, fl, com)
                                                     for t, rm, s, fl, com in bs])
    """

    def __init__(self, capacity: int):
        if (not isinstance(capacity, (int, np.integer)) or isinstance(capacity, (bool, np.bool_))
                or not 1 <= int(capacity) <= MAX_CAPACITY):
            raise ValueError(f"roster capacity must be an int in [1, {MAX_CAPACITY}], not {capacity!r}")
        self.capacity = int(capacity)
        # the host mirror, as nd_roster_fanout takes it: `capacity` int32 rooms (-1: none), then `capacity` flag bytes
        self._table = np.zeros(5 * self.capacity, dtype=np.uint8)
        self._room = self._table[:4 * self.capacity].view(np.int32)
        self._flags = self._table[4 * self.capacity:]
        self._room[:] = -1
        self._dirty = True
        self._handle = None
        self._closed = False

    def _check_open(self) -> None:
        if self._closed:
            raise ValueError("the roster is closed")

    def _slot(self, v) -> int:
        if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)) or not 0 <= int(v) < self.capacity:
            raise ValueError(f"slot must be an int in [0, {self.capacity}), not {v!r}")
        return int(v)

    def update(self, slots, *, room=_KEEP, login=_KEEP, ignall=_KEEP, ignshout=_KEEP, colour=_KEEP) -> None:
        """Set fields of ``slots`` (a slot or a sequence of them).  Each field given is one value for every slot or a
        sequence of one per slot; a field not given stays as it is.  ``room`` is None (no room) or an int in
        [0, ROOM_LIMIT); the flags are 0/1 or bools.  A slot given more than once takes its last values.  Nothing
        changes unless the whole update is valid."""
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
        _, last = np.unique(idx[::-1], return_index=True)        # each slot's last position: last write wins
        keep = n - 1 - last
        at = idx[keep]
        if rooms is not None:
            self._room[at] = rooms[keep]
        for f, v in flags.items():
            bit = np.uint8(ROSTER_FLAGS[f])
            self._flags[at] = np.where(v[keep] != 0, self._flags[at] | bit, self._flags[at] & ~bit)
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
        text_off = np.zeros(len(texts), dtype=np.int32)
        np.cumsum(lens[:-1], out=text_off[1:])
        return (b"".join(texts), text_off, lens.astype(np.int32), np.array(rms, dtype=np.int32),
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

    def _prepare_plan(self, broadcasts):
        """As _prepare, for nd_roster_plan: there is no arena, so its bound does not apply; the variant buffer's does
        (12 * text bytes + 16 * K at most MANY_ARENA_CAP), and K x bitmap words stays below 2^31."""
        checked = self._checked(broadcasts, (self.capacity + 63) // 64, "K x ceil(capacity / 64)")
        lens = checked[1]
        bound = 12 * int(lens.sum()) + 16 * len(lens)
        if bound > MANY_ARENA_CAP:
            raise ValueError(f"call too large: its variant bound (12 x text bytes + 16 x K) is {bound} bytes, the cap "
                             f"is {MANY_ARENA_CAP} (MANY_ARENA_CAP): split it")
        return self._packed(*checked)

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
        if rc != 0:
            raise RuntimeError(f"device fan-out failed: {lib.nd_last_error().decode(errors='replace')}")
        self._dirty = False
        r = _result(lib, admitted, out_off, w_off, t)
        r.timing.update(h2d_bytes=t.h2d_bytes, d2h_bytes=t.d2h_bytes)
        r.broadcast_offsets = np.arange(k + 1, dtype=np.int64) * self.capacity
        return r

    def _device_handle(self, lib) -> int:
        if self._handle is None:
            h = lib.nd_roster_create(self.capacity)
            if h < 0:
                raise RuntimeError(f"cannot create a device roster: {lib.nd_last_error().decode(errors='replace')}")
            self._handle = h
        return self._handle

    def plan_many(self, broadcasts) -> Plan:
        """The delivery plan of K broadcasts to this roster, in one device call: what :meth:`broadcast_many` takes,
        checked by the same rules, except that no arena bound applies; instead the variant bound, 12 x the call's text
        bytes + 16 x K, must not exceed MANY_ARENA_CAP.  One upload, one kernel, one download, one synchronise,
        whatever K and the capacity.  The contract::

            roster.plan_many(bs).expand() == roster.broadcast_many(bs)
        """
        self._check_open()
        text, text_off, lens, rm, sender, flags, coms = self._prepare_plan(broadcasts)
        lib = _load()
        handle = self._device_handle(lib)
        k, words = len(lens), (self.capacity + 63) // 64
        bits = np.empty((k, words), dtype=np.uint64)
        vn = np.empty((k, 2), dtype=np.int64)
        vw = np.empty((k, 2), dtype=np.int32)
        vwsz = np.empty((k, 2, MAX_WRITES), dtype=np.int32)
        var = np.empty(12 * len(text) + 16 * k, dtype=np.uint8)
        tbuf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        t = _RosterTiming()
        rc = lib.nd_roster_plan(handle, k, _ptr(tbuf), len(text), _ptr(text_off), _ptr(lens), _ptr(rm), _ptr(sender),
                                _ptr(flags), _ptr(coms), _ptr(self._table) if self._dirty else None, _ptr(bits),
                                _ptr(vn), _ptr(vw), _ptr(vwsz), _ptr(var), ctypes.byref(t))
        if rc != 0:
            raise RuntimeError(f"device plan failed: {lib.nd_last_error().decode(errors='replace')}")
        self._dirty = False
        # the variant buffer's layout (var_at / var_stride of fanout.hip): two 4-byte aligned slots per broadcast
        starts = np.empty((k, 2), dtype=np.int64)
        starts[:, 0] = 12 * text_off.astype(np.int64) + 16 * np.arange(k, dtype=np.int64)
        starts[:, 1] = starts[:, 0] + ((6 * lens.astype(np.int64) + 4 + 3) & ~3)
        return Plan(capacity=self.capacity, admitted_bits=bits,
                    colour_bits=_pack((self._flags & ROSTER_FLAGS["colour"]) != 0), variants=var,
                    variant_starts=starts, variant_sizes=vn, write_counts=vw, write_sizes=vwsz,
                    timing={"kernels_us": t.kernels_us, "end_to_end_us": t.end_to_end_us, "h2d_bytes": t.h2d_bytes,
                            "d2h_bytes": t.d2h_bytes})

    def close(self) -> None:
        """Free the device table; the roster cannot be used afterwards.  Closing twice is harmless."""
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
