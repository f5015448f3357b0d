"""Many broadcasts in one device call: ``device.broadcast_many`` and nuts_fanout_{measure,emit}_many of fanout.hip.

Host tier (unmarked): the new kernels compile for gfx950 with no scratch, no spills and no dynamic stack; malformed
calls are rejected before the device library loads; ``broadcast_offsets`` and ``Fanout.item`` address items by
(broadcast, listener).

GPU tier: everything that touches the device runs in ONE short-lived child for the module (tests/device_many_child.py,
under ``timeout``), as tests/test_device_fanout.py does, and the tests assert on its JSON: seeded random calls of
K in {1, 2, 7, 64, 300, 1000} broadcasts against the CPU restatement, the same broadcasts one ``broadcast()`` at a time,
the bench step's shape, the worst case with buffer reuse, and the timing fields.
"""
from __future__ import annotations

import json
import re
import subprocess

import numpy as np
import pytest

import child_run
from nuts333_amd import device

MANY_KERNELS = ("nuts_fanout_measure_many", "nuts_fanout_emit_many")


# ------------------------------------------------------------------ host tier
def test_many_kernels_compile_for_gfx950_without_scratch(tmp_path):
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
    for name in MANY_KERNELS:
        assert name in device.KERNELS
        u = usage.get(name)
        assert u is not None, f"kernel {name} missing from the resource report"
        assert u.get("ScratchSize [bytes/lane]") == "0", (name, u)
        assert u.get("VGPRs Spill") == "0" and u.get("SGPRs Spill") == "0", (name, u)
        assert u.get("Dynamic Stack") == "False", (name, u)


def _no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


LISTENER = [0, 1, 1, 0, 0, 0, 1]
GOOD = (b"hi\n", [LISTENER], 0, 0, device.COM_SAY)


@pytest.mark.parametrize("call", [
    [],                                          # no broadcasts
    (),
    np.zeros((0, 5)),
    b"hi\n",                                     # not a sequence of tuples
    42,
    [(b"hi\n", [LISTENER], 0, 0)],               # four fields
    [GOOD + (0,)],                               # six
    [list(GOOD)],                                # not a tuple
    [b"hi\n"],
    [GOOD, (b"hi\n", [LISTENER])],               # a bad shape among good ones
])
def test_broadcast_many_rejects_malformed_calls_before_the_device(monkeypatch, call):
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        device.broadcast_many(call)


# each kind of input broadcast() rejects (tests/test_device_fanout.py), as one bad tuple between two good ones
@pytest.mark.parametrize("bad", [
    (b"hi\n", [], 0, 0, 3),                                      # no listeners
    (b"hi\n", np.zeros((0, 7), dtype=int), 0, 0, 3),
    (b"hi\n", [[0, 1, 1, 0, 0, 0]], 0, 0, 3),                    # six columns: colour missing
    (b"hi\n", [LISTENER, [0, 1]], 0, 0, 3),                      # ragged
    (b"hi\n", [[0, 1, 1, 0, 0, 0, 2]], 0, 0, 3),                 # a field that is not 0/1
    (b"hi\n", [[0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0]], 0, 0, 3),   # not integers
    (b"hi\n", [LISTENER], 2, 0, 3),                              # rm_is_null not a flag
    (b"hi\n", [LISTENER], 0, 7, 3),                              # force_listen not a flag
    (b"hi\n", [LISTENER], 0, 0, 92),                             # no such command
    (b"hi\n", [LISTENER], 0, 0, -1),
    (b"h\0i\n", [LISTENER], 0, 0, 3),                            # NUL
    (b"y" * 2000, [LISTENER], 0, 0, 4),                          # too long
    ("caf€", [LISTENER], 0, 0, 3),                          # not one byte per character
    (42, [LISTENER], 0, 0, 3),                                   # not text
])
def test_broadcast_many_rejects_one_bad_broadcast_among_good_ones(monkeypatch, bad):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match=r"^broadcast 1: "):
        device.broadcast_many([GOOD, bad, GOOD])


def test_broadcast_many_rejects_a_call_over_the_cap(monkeypatch):
    _no_library(monkeypatch)
    text = b"\n" * 1999
    n = device.MANY_ARENA_CAP // device.max_bytes(len(text))          # the most listeners at the cap
    table = np.zeros((n + 1, 7), dtype=np.uint8)
    with pytest.raises(ValueError, match="MANY_ARENA_CAP"):
        device.broadcast_many([(text, table, 0, 0, device.COM_SAY)])
    half = table[:n // 2 + 1]                                        # over the cap only together
    with pytest.raises(ValueError, match="MANY_ARENA_CAP"):
        device.broadcast_many([(text, half, 0, 0, device.COM_SAY), (text, half, 0, 0, device.COM_SHOUT)])
    # at the cap the call is packed, not refused
    packed = device._prepare_many([(text, table[:n], 0, 0, device.COM_SAY)])
    assert len(packed[-1]) == n and n * device.max_bytes(len(text)) <= device.MANY_ARENA_CAP


def test_prepare_many_packs_texts_flags_commands_and_item_offsets():
    text, text_off, lens, flags, coms, item_off, rec = device._prepare_many([
        (b"ab\n", [LISTENER, [1] * 7], 1, 0, device.COM_SHOUT),
        ("", [[0] * 7], 0, 1, device.COM_SAY),
        (b"xyz", [LISTENER] * 3, 1, 1, device.COM_SEMOTE),
    ])
    assert text == b"ab\nxyz" and text_off.tolist() == [0, 3, 3] and lens.tolist() == [3, 0, 3]
    assert flags.tolist() == [1, 2, 3] and coms.tolist() == [device.COM_SHOUT, device.COM_SAY, device.COM_SEMOTE]
    assert item_off.tolist() == [0, 2, 3, 6] and item_off.dtype == np.int32
    assert rec.tolist() == [2 | 4 | 64, 127, 0] + [2 | 4 | 64] * 3


def test_broadcast_offsets_address_items_by_broadcast_and_listener():
    # broadcast 0: listeners 0 (b"ab", one write) and 1 (not admitted); broadcast 1: listener 0 (b"XYZ" in 2 writes);
    # broadcast 2: listener 0 (b"q")
    r = device.Fanout(admitted=np.array([True, False, True, True]), out_offsets=np.array([0, 2, 2, 5, 6]),
                      arena=np.frombuffer(b"abXYZq", dtype=np.uint8), write_offsets=np.array([0, 1, 1, 3, 4]),
                      write_sizes=np.array([2, 1, 2, 1], dtype=np.int32), broadcast_offsets=np.array([0, 2, 3, 4]))
    assert [r.item(0, 0), r.item(0, 1), r.item(1, 0), r.item(2, 0)] == [0, 1, 2, 3]
    assert device.chunks(r, r.item(0, 0)) == [b"ab"] and device.chunks(r, r.item(0, 1)) == []
    assert device.chunks(r, r.item(1, 0)) == [b"X", b"YZ"] and r.output(r.item(2, 0)) == b"q"
    for k, j in ((1, 1), (3, 0), (-1, 0), (0, -1), (0, 2)):
        with pytest.raises(IndexError):
            r.item(k, j)
    single = device.Fanout(admitted=np.array([True]), out_offsets=np.array([0, 1]), arena=np.frombuffer(b"a", np.uint8),
                           write_offsets=np.array([0, 1]), write_sizes=np.array([1], dtype=np.int32))
    assert single.broadcast_offsets is None
    with pytest.raises(ValueError):
        single.item(0, 0)


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def many_run(built):
    res = child_run.run_child("device_many_child.py", "DEVICE_MANY", 900)
    print("\n[broadcast_many]", json.dumps(res)[:1500])
    return res


@pytest.mark.gpu
def test_random_calls_match_the_cpu_restatement(many_run):
    r = many_run["random"]
    assert sorted(set(r["ks"])) == [1, 2, 7, 64, 300, 1000]
    assert r["broadcasts"] >= 2000 and r["items"] >= 500_000
    assert r["records_seen"] == 128 and r["long_texts"] > 0        # every listener record; texts past 994 bytes
    assert r["n_bad"] == 0, r["first_bad"]


@pytest.mark.gpu
def test_many_equals_one_broadcast_per_call_slice_by_slice(many_run):
    s = many_run["singles"]
    assert s["broadcasts"] == 1 + 2 + 7 + 64 + 300 + 1000 and s["items"] > 0
    assert s["n_bad"] == 0, s["first_bad"]


@pytest.mark.gpu
def test_bench_step_of_100_shouts_to_1000_listeners(many_run):
    b = many_run["bench_step"]
    assert b["broadcasts"] == 100 and b["deliveries"] == 99_900
    assert b["n_bad"] == 0, b["first_bad"]


@pytest.mark.gpu
def test_worst_case_items_and_buffer_reuse(many_run):
    w = many_run["worst"]
    assert w["items"] == 64 * 64 and w["per_item"] == [[11_998, 14]]
    assert w["n_bad"] == 0, w["first_bad"]
    assert w["reuse_identical"] is True


@pytest.mark.gpu
def test_timing_fields_are_present(many_run):
    t = many_run["bench_step"]["timing"]
    assert 0 < t["kernels_us"] <= t["end_to_end_us"]
