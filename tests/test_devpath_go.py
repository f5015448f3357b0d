"""``python -m nuts333_amd.devpath --go K[,K...]``: go_many timed beside the parts it is made of and beside the CPU.

Host tier: the option rejects what ``--per-call`` rejects; with no GPU visible the command still exits 2 and measures
nothing; the call the command models for the CPU -- the deferral rule, the reference's formats, ``look()``'s strings -- is
what the model of tests/device_go_child.py answers for the roster the command builds, there and back.
GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``, prints one line whose
``go`` section has a case per colour and K with the device's times, the parts' and the CPU's.  No time is a pass condition.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import child_run
from device_go_child import go_call, go_user, look_of
from device_rooms_child import list_room
from nuts333_amd import device, devpath, nuts_path
from nuts333_amd.provision import SIX_ROOMS


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "x", "", "1,,2", "2.5"])
def test_go_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--go", value])
    assert e.value.code == 2
    assert "argument --go:" in capsys.readouterr().err


def test_go_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "go_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--go", "1,8"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_go_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.go_cases([1], 1, 0, {})


def test_the_call_handed_to_the_cpu_is_the_models():
    n = 1000
    names, accesses = devpath.ROOMS_LISTS["6"]
    label = {r.label: i for i, r in enumerate(SIX_ROOMS)}
    assert [[label[l] for l in r.links] for r in SIX_ROOMS] == [list(l) for l in devpath.GO_LINKS]
    assert all(h in devpath.GO_LINKS[t] and t in devpath.GO_LINKS[h] for h, t in enumerate(devpath.GO_THERE))
    rms = [list_room(name, access=access, links=list(links)) for name, access, links in zip(names, accesses, devpath.GO_LINKS)]
    users = {j: go_user(j, name=b"User%d" % j, room=j % 6, level=2) for j in range(n)}
    room_of = np.arange(n) % 6
    for k in (1, 8, 64):
        movers = list(range(k))
        for events in ([(j, names[devpath.GO_THERE[j % 6]], 2) for j in movers], [(j, names[j % 6], 2) for j in movers]):
            got = devpath.go_model(room_of, events)
            call = go_call(users, rms, [], events, 3, 2)
            assert [g[0] for g in got] == [e["outcome"] for e in call["events"]]
            for g, e in zip(got, call["events"]):
                if e["outcome"] != device.GO_DEFERRED:
                    assert g[1:] == (e["target"], e["enter"], e["leave"], e["reply"])
            for j in call["movers"]:
                assert [ch for s in devpath.go_look_strings(room_of, j) for ch in nuts_path.chunks(s, 0)] == look_of(users, rms, j)
        assert room_of.tolist() == [j % 6 for j in range(n)]              # there and back: the state is periodic
    assert sum(g[0] == device.GO_WALKED for g in devpath.go_model(room_of.copy(), [(j, names[devpath.GO_THERE[j % 6]], 2) for j in range(64)])) == 2


@pytest.mark.gpu
def test_devpath_go_prints_one_line_with_the_parts_and_the_cpu(built):
    j = child_run.run_devpath("devpath --go", 300, "--go", "1,8", "--reps", "3", "--warmup", "1", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and not {"plan", "roster", "look", "relay", "who", "rooms"} & set(j)
    assert j["go_kernels"][:2] == list(device.GO_KERNELS) and j["go_end_to_end_covers"] and j["go_parts_covers"] and j["go_cpu_us_covers"]
    gs = j["go"]
    assert [(c["colour"], c["k"]) for c in gs] == [(colour, k) for colour in devpath.COLOURS for k in (1, 8)]
    for c in gs:
        assert c["n"] == 1000 and c["rooms"] == 6 and c["moved"] + c["deferred"] + c["already"] == c["k"] and c["moved"] == min(c["k"], 2)
        assert c["back_moved"] == c["moved"] and c["back_moved"] + c["back_already"] + c["back_deferred"] == c["k"]
        assert 0 < c["kernels_us"]["median"] <= c["end_to_end_us"]["median"] <= c["python_us"]["median"] and c["bytes_out"] > 0
        assert c["cpu_us"]["median"] > 0 and c["end_to_end_over_cpu"] > 0 and c["parts"]["end_to_end_us"]["median"] > 0
        # the events go up with the first visit and the table, 5 bytes a slot in two 256-byte slices, with the look
        assert 4096 + 1024 < c["h2d_bytes"] < 2 * (4096 + 1024) and c["parts"]["h2d_bytes"] < 4096 + 1024 and c["back"]["h2d_bytes"] > 4096 + 1024
    print("\n[devpath --go]", json.dumps(gs)[:3000])
