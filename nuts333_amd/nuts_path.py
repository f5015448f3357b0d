"""The ctypes binding of oracle/nuts_path.h, the CPU restatement of the path (``oracle/_build/libnuts_path.so``).

The one Python module that knows the library's C ABI: a signature for every ``np_*`` function of the header, the
``struct np_listener`` and ``struct np_stage`` layouts and the ``np_emit_fn`` callback type.  ``lib()`` loads the
library once, running ``make -C oracle port`` first when it is missing; the helpers below are the calls that the tests
and ``nuts333_amd.devpath`` repeat.  (``bench.py`` keeps a binding of its own.)
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
LIBRARY = REPO / "oracle" / "_build" / "libnuts_path.so"


class Listener(ctypes.Structure):
    """struct np_listener: what the fan-out predicate reads of one listener (nuts333.c:1410-1415)."""
    _fields_ = [(f, ctypes.c_int) for f in ("login", "has_room", "same_room", "ignall", "ignshout", "is_sender")]


class Stage(ctypes.Structure):
    """struct np_stage: the write_user staging buffer (NP_OUT_BUFF + 8 bytes) and its fill level."""
    _fields_ = [("buff", ctypes.c_char * 1008), ("pos", ctypes.c_int)]


#: np_emit_fn: called once per write(2) the reference issues, with that write's bytes
EMIT = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_char), ctypes.c_size_t)

_str, _int, _size, _ptr = ctypes.c_char_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
#: name -> (restype, argtypes), in the order of oracle/nuts_path.h.  Output buffers are ``char *``: pass a
#: ``ctypes.create_string_buffer``.
SIGNATURES = {
    "np_terminate": (_int, [_str]),
    "np_wordfind": (_int, [_str, _str]),                 # words: char[NP_MAX_WORDS][NP_WORD_LEN + 1]
    "np_remove_first": (_str, [_str]),
    "np_command_count": (_int, []),
    "np_command_name": (_str, [_int]),
    "np_command_level": (_int, [_int]),
    "np_command_lookup": (_int, [_str]),
    "np_stage_init": (None, [ctypes.POINTER(Stage)]),
    "np_stage_feed": (None, [ctypes.POINTER(Stage), _str, _int, EMIT, _ptr]),
    "np_stage_flush": (None, [ctypes.POINTER(Stage), EMIT, _ptr]),
    "np_write_user_stream": (None, [_str, _int, EMIT, _ptr]),
    "np_transduce": (_size, [_str, _int, _str, _size]),
    "np_write_count": (_int, [_str, _int]),
    "np_colour_com_strip": (_size, [_str, _str, _size]),
    "np_colour_code": (_str, [_int]),
    "np_colour_com": (_str, [_int]),
    "np_say_verb": (_str, [_str]),
    "np_contains_swearing": (_int, [_str]),
    "np_fanout_admits": (_int, [ctypes.POINTER(Listener), _int, _int, _int]),
    "np_record": (None, [_str, _int, ctypes.POINTER(_int), _str]),   # ring: nlines x (NP_REVIEW_LEN + 2)
}

_LIB = None


def build() -> None:
    """``make -C oracle port``: the restatement's library, its talker and pathbench."""
    subprocess.run(["make", "-s", "-C", str(REPO / "oracle"), "port"], check=True)


def lib() -> ctypes.CDLL:
    """The library with every function of the header typed (built first if it is missing)."""
    global _LIB
    if _LIB is None:
        if not LIBRARY.exists():
            build()
        so = ctypes.CDLL(str(LIBRARY))
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(so, name)
            fn.restype, fn.argtypes = restype, argtypes
        _LIB = so
    return _LIB


def transduce(text: bytes, colour: int) -> bytes:
    """np_transduce: every byte a listener with this colour bit receives for ``text``."""
    n = lib().np_transduce(text, colour, None, 0)
    out = ctypes.create_string_buffer(n)
    lib().np_transduce(text, colour, out, n)
    return out.raw


def write_count(text: bytes, colour: int) -> int:
    """np_write_count: the write(2) calls the reference makes for ``text``."""
    return lib().np_write_count(text, colour)


def chunks(text: bytes, colour: int) -> list[bytes]:
    """np_write_user_stream: the bytes of each write(2) the reference makes for ``text``, in order."""
    out: list[bytes] = []
    lib().np_write_user_stream(text, colour, EMIT(lambda ctx, buf, n: out.append(ctypes.string_at(buf, n))), None)
    return out


def admits(fields, rm_is_null: int, force_listen: int, com_num: int) -> bool:
    """np_fanout_admits for a listener given as the six fields of struct np_listener, in order."""
    return bool(lib().np_fanout_admits(ctypes.byref(Listener(*fields)), rm_is_null, force_listen, com_num))
