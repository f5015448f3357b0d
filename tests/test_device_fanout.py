"""The device fan-out kernel (nuts333_amd/device/fanout.hip) against the CPU restatement.

Host tier (unmarked): the .hip compiles for gfx950 with no scratch; the Python API rejects malformed input before it
loads the device library; the hard size / write bounds the library allocates by hold on the CPU restatement at their
worst cases.

GPU tier: everything that touches the device runs in ONE short-lived child per module (tests/device_fanout_child.py,
under ``timeout``; DESIGN.md section 7: a process that boots talkers never initialises HIP) and the tests assert on its
JSON -- the 314 transducer vectors, >= 200k seeded fuzz strings (bytes and write(2) chunk sizes against
``np_write_user_stream``), the admit predicate's full truth table and a 1000-listener broadcast.
"""
from __future__ import annotations

import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import child_run
from nuts333_amd import device, nuts_path

REPO = Path(__file__).resolve().parent.parent
FUZZ = 200_000


# ------------------------------------------------------------------ host tier
def test_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    cc = device.hipcc()
    if cc is None:
        pytest.skip("hipcc not installed")
    p = subprocess.run([cc, "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        str(device.SOURCE), "-o", str(tmp_path / "lib.so")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    report = p.stdout.decode(errors="replace")
    assert p.returncode == 0, report[-2000:]
    usage, current = {}, None
    for line in report.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            current = m.group(1)
            usage[current] = {}
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|Dynamic Stack): (\S+)", line)
        if m and current:
            usage[current][m.group(1)] = m.group(2)
    for k in device.KERNELS:
        assert k in usage, f"kernel {k} missing from the resource report"
    assert len(usage) > len(device.KERNELS)          # the rocPRIM scan kernels are in the same report
    for name, u in usage.items():
        assert u.get("ScratchSize [bytes/lane]") == "0", (name, u)
        assert u.get("VGPRs Spill", "0") == "0" and u.get("SGPRs Spill", "0") == "0", (name, u)
        assert u.get("Dynamic Stack", "False") == "False", (name, u)


def _no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


LISTENER = [0, 1, 1, 0, 0, 0, 1]


@pytest.mark.parametrize("texts, colours", [
    ([], []),                                    # empty batch
    ([b"hello\0world\n"], [0]),                  # NUL inside a text
    (["x" * 2000], [1]),                         # NP_TEXT_SIZE or more
    ([b"a" * 5000], [0]),
    (["caf€"], [0]),                        # not one byte per character
    ([b"ok\n", b"ok\n"], [0]),                   # colour bits do not match the texts
    ([b"ok\n"], [2]),                            # a colour bit that is not a bit
    ([42], [0]),                                 # not text
])
def test_transduce_batch_rejects_malformed_input_before_the_device(monkeypatch, texts, colours):
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        device.transduce_batch(texts, colours)


@pytest.mark.parametrize("text, listeners, args", [
    (b"hi\n", [], (0, 0, 3)),                                   # no listeners
    (b"hi\n", np.zeros((0, 7), dtype=int), (0, 0, 3)),
    (b"hi\n", [[0, 1, 1, 0, 0, 0]], (0, 0, 3)),                 # six columns: colour missing
    (b"hi\n", [LISTENER, [0, 1]], (0, 0, 3)),                   # ragged
    (b"hi\n", [[0, 1, 1, 0, 0, 0, 2]], (0, 0, 3)),              # a field that is not 0/1
    (b"hi\n", [[0, 1, 1, 0, 0, 0, -1]], (0, 0, 3)),
    (b"hi\n", [[0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0]], (0, 0, 3)),   # not integers
    (b"hi\n", [LISTENER], (2, 0, 3)),                            # rm_is_null not a flag
    (b"hi\n", [LISTENER], (0, 7, 3)),                            # force_listen not a flag
    (b"hi\n", [LISTENER], (0, 0, 92)),                           # no such command
    (b"hi\n", [LISTENER], (0, 0, -1)),
    (b"h\0i\n", [LISTENER], (0, 0, 3)),                          # NUL
    (b"y" * 2000, [LISTENER], (0, 0, 4)),                        # too long
])
def test_broadcast_rejects_malformed_input_before_the_device(monkeypatch, text, listeners, args):
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        device.broadcast(text, listeners, *args)


def test_listener_records_pack_one_byte_per_listener():
    rec = device._listener_records([[1, 0, 0, 0, 0, 0, 0], [0, 1, 1, 0, 1, 0, 1], [1] * 7])
    assert rec.dtype == np.uint8 and rec.tolist() == [1, 2 | 4 | 16 | 64, 127]


def test_chunks_helper_splits_an_item_by_its_write_sizes():
    r = device.Fanout(admitted=np.array([True, False, True]), out_offsets=np.array([0, 5, 5, 8]),
                      arena=np.frombuffer(b"abcdeXYZ", dtype=np.uint8), write_offsets=np.array([0, 2, 2, 3]),
                      write_sizes=np.array([3, 2, 3], dtype=np.int32))
    assert device.chunks(r, 0) == [b"abc", b"de"] and device.chunks(r, 1) == [] and device.chunks(r, 2) == [b"XYZ"]


def test_size_and_write_bounds_hold_on_the_cpu_restatement():
    """The bounds the device library allocates by: 6*len + 4 bytes and MAX_WRITES writes per item of len < 2000."""
    worst = b"\n" * 1999
    assert len(nuts_path.transduce(worst, 1)) == 11_998 == device.max_bytes(1999)
    assert nuts_path.write_count(worst, 1) == 14 <= device.MAX_WRITES
    codes = b"~RS" * 666
    assert nuts_path.transduce(codes, 0) == b"" and nuts_path.write_count(codes, 0) == 0
    sys.path.insert(0, str(REPO / "tests"))
    import device_fanout_child as child
    for text, _ in child.fuzz_items(7, 3000) + [(b"~" * 1999, 0), (b"/~" * 999 + b"\n", 1), (b"~FR\n" * 499, 1)]:
        for colour in (0, 1):
            assert len(nuts_path.transduce(text, colour)) <= device.max_bytes(len(text)), text
            assert nuts_path.write_count(text, colour) <= device.MAX_WRITES, text


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def device_run(built):
    res = child_run.run_child("device_fanout_child.py", "DEVICE_FANOUT", 900, "--fuzz", str(FUZZ))
    print("\n[device fan-out]", json.dumps({k: v for k, v in res.items() if k != "vectors"})[:1500])
    return res


@pytest.mark.gpu
def test_device_transduces_the_314_reference_vectors(device_run):
    v = device_run["vectors"]
    assert v["vectors"] == 314 and v["items"] == 628
    assert v["n_concat_bad"] == 0, v["concat_bad"]
    assert v["n_chunk_bad"] == 0


@pytest.mark.gpu
def test_device_matches_np_write_user_stream_on_seeded_fuzz(device_run):
    f = device_run["fuzz"]
    assert f["items"] == FUZZ >= 200_000
    assert f["n_bad"] == 0, f["first_bad"]
    assert f["writes"] > f["items"] // 2        # colour on writes twice: the chunking was exercised, not just bytes
    assert f["max_bytes_minus_bound"] <= 0 and f["max_writes"] <= device.MAX_WRITES


@pytest.mark.gpu
def test_device_worst_cases_stay_within_the_bounds(device_run):
    w = device_run["worst"]
    assert w["n_bad"] == 0, w["first_bad"]
    assert w["newlines_colour_on"] == [11_998, 14]
    assert w["codes_colour_off"] == [0, 0]


@pytest.mark.gpu
def test_device_admit_predicate_matches_its_full_truth_table(device_run):
    p = device_run["predicate"]
    assert p["cases"] == 64 * 2 * 2 * 3
    assert p["n_bad"] == 0, p["first_bad"]


@pytest.mark.gpu
def test_device_1000_listener_broadcast_matches_the_cpu_loop(device_run):
    b = device_run["broadcast"]
    assert b["listeners"] == 1000 and b["n_bad"] == 0
    assert b["admitted"] == b["cpu_admitted"] and 0 < b["admitted"] < 1000 and b["sender_admitted"] is False
    assert b["timing"]["kernels_us"] > 0 and b["timing"]["end_to_end_us"] >= b["timing"]["kernels_us"]


def test_command_numbers_match_the_restatement():
    lib = nuts_path.lib()
    assert device.NUM_COMMANDS == lib.np_command_count()
    assert (device.COM_SAY, device.COM_SHOUT, device.COM_SEMOTE) == tuple(
        lib.np_command_lookup(w) for w in (b"say", b"shout", b"semote"))
    # the listener record's first six columns are struct np_listener, field for field, in the header and the binding
    body = re.search(r"struct np_listener \{(.*?)\};", (REPO / "oracle" / "nuts_path.h").read_text(), re.S).group(1)
    header_fields = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert [f for f, _ in nuts_path.Listener._fields_] == header_fields == list(device.LISTENER_FIELDS[:6])
