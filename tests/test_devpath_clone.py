"""``python -m nuts333_amd.devpath --clone K[,K...]``: clone_many timed beside speak_many of the same bodies and beside the CPU.

Host tier: the option rejects what ``--per-call`` rejects; with no GPU visible the command still exits 2 and measures
nothing; the events the command submits -- K ``.csay`` events by K owners, K ``.clone`` events and K ``.destroy`` events --
are answered by the model of tests/device_clone_child.py as the command expects, and the ``.destroy`` call ends where the
``.clone`` call began.
GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``, prints one line whose
``clone`` section has a case per colour and K with the device's times, ``speak_many``'s and the CPU's.  No time is a pass
condition but their order: the kernels within the call, the call within the Python call.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import child_run
from device_clone_child import clone_call
from device_go_child import go_user
from device_rooms_child import list_room
from nuts333_amd import device, devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "x", "", "1,,2", "2.5"])
def test_clone_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--clone", value])
    assert e.value.code == 2
    assert "argument --clone:" in capsys.readouterr().err


def test_clone_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "clone_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--clone", "1,8"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_clone_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.clone_cases([1], 1, 0, {})


def test_the_calls_the_command_submits_are_answered_as_it_expects():
    n, most = 1000, 64
    names, accesses = devpath.ROOMS_LISTS["6"]
    room_of = np.arange(n) % 6
    for k in (1, 8, 64):
        rms = [list_room(name, access=access, links=list(links)) for name, access, links in zip(names, accesses, devpath.GO_LINKS)]
        users = {j: go_user(j, name=b"User%d" % j, room=j % 6, level=3, muzzled=0) for j in range(n)}
        start = [(j, j % 6, device.CLONE_HEAR_ALL) for j in range(most)] + [None] * most
        clones = list(start)
        csays, lines = devpath.clone_csays(k, names)
        call = clone_call(users, rms, clones, csays, 2, 3, 2)
        assert [e["outcome"] for e in call["events"]] == [device.CLONE_SAID] * k and [e["said"] for e in call["events"]] == lines
        assert [e["record"] for e in call["events"]] == list(range(k)) and len({ev[0] for ev in csays}) == k
        actors = list(range(most, most + k))
        made = clone_call(users, rms, clones, [(j, device.COM_CLONE, b"", 1) for j in actors], 2, 3, 2)
        assert [e["outcome"] for e in made["events"]] == devpath.clone_model(room_of, actors, False)
        assert sum(e["outcome"] == device.CLONE_CREATED for e in made["events"]) == min(k, 6) and clones != start
        gone = clone_call(users, rms, clones, [(j, device.COM_DESTROY, b"", 1) for j in actors], 2, 3, 2)
        assert [e["outcome"] for e in gone["events"]] == devpath.clone_model(room_of, actors, True)
        assert clones == start and [rm["access"] for rm in rms] == list(accesses)      # periodic


@pytest.mark.gpu
def test_devpath_clone_prints_one_line_with_the_parts_and_the_cpu(built):
    j = child_run.run_devpath("devpath --clone", 300, "--clone", "1,8", "--reps", "3", "--warmup", "1", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and not {"plan", "roster", "look", "relay", "who", "rooms", "go", "access"} & set(j)
    assert j["clone_kernels"][:2] == list(device.CLONE_KERNELS) and j["clone_end_to_end_covers"] and j["clone_speak_covers"]
    assert j["clone_cpu_us_covers"]
    cs = j["clone"]
    assert [(c["colour"], c["k"]) for c in cs] == [(colour, k) for colour in devpath.COLOURS for k in (1, 8)]
    for c in cs:
        assert c["n"] == 1000 and c["rooms"] == 6 and c["records"] == 16 and c["created"] == min(c["k"], 6) == c["k"] - c["deferred"]
        for step in (c, c["speak"], c["clone"], c["destroy"]):
            assert 0 < step["kernels_us"]["median"] <= step["end_to_end_us"]["median"] <= step["python_us"]["median"]
        # the events alone; with the clone records, three 256-byte slices, in the calls that follow a change of theirs; never
        # the 5 bytes a slot of the table
        assert c["h2d_bytes"] < 4096 and c["speak"]["h2d_bytes"] < 4096
        assert 768 < c["clone"]["h2d_bytes"] < 768 + 4096 and 768 < c["destroy"]["h2d_bytes"] < 768 + 4096
        assert c["cpu_us"]["median"] > 0 and c["end_to_end_over_cpu"] > 0
        assert all(v > 0 for v in c["csay_over_speak"].values())
        assert all(lo <= c["csay_over_speak"][f] <= hi for f, (lo, hi) in c["csay_over_speak_p10_p90"].items())
    print("\n[devpath --clone]", json.dumps(cs)[:3000])
