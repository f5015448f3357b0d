"""``python -m nuts333_amd.devpath --access K[,K...]``: access_many timed beside plan_many of its lines and beside the CPU.

Host tier: the option rejects what ``--per-call`` rejects; with no GPU visible the command still exits 2 and measures
nothing; the call the command models for the CPU -- the deferral rule and the reference's formats -- is what the model of
tests/device_access_child.py answers for the roster the command builds, the ``.private`` call and the ``.public`` call after it.
GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``, prints one line whose
``access`` section has a case per colour and K with the device's times, ``plan_many``'s and the CPU's.  No time is a pass
condition but their order: the kernels within the call, the call within the Python call.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import child_run
from device_access_child import access_call
from device_go_child import go_user
from device_rooms_child import list_room
from nuts333_amd import device, devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "x", "", "1,,2", "2.5"])
def test_access_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--access", value])
    assert e.value.code == 2
    assert "argument --access:" in capsys.readouterr().err


def test_access_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "access_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--access", "1,8"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_access_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.access_cases([1], 1, 0, {})


def test_the_call_handed_to_the_cpu_is_the_models():
    n = 1000
    names, accesses = devpath.ROOMS_LISTS["6"]
    rms = [list_room(name, access=access, links=list(links)) for name, access, links in zip(names, accesses, devpath.GO_LINKS)]
    users = {j: go_user(j, name=b"User%d" % j, room=j % 6, level=1) for j in range(n)}
    room_of = np.arange(n) % 6
    state = list(accesses)
    for k in (1, 8, 64):
        actors = devpath.access_actors(k, n)
        assert len(actors) == k and [int(room_of[j]) for j in actors[:3]] == [3, 4, 5][:k]
        for com in (device.COM_PRIVATE, device.COM_PUBLIC):              # the .private call, then the .public call: there and back
            events = [(j, com, b"", 1) for j in actors]
            got = devpath.access_model(state, room_of, events)
            call = access_call(users, rms, [], events, 3, 2, 2)
            assert [g[0] for g in got] == [e["outcome"] for e in call["events"]]
            for g, e in zip(got, call["events"]):
                if e["outcome"] != device.ACCESS_DEFERRED:
                    assert g[1:] == (e["target_room"], e["reply"], e["here"]) and e["there"] is None and e["notice"] is None
            assert state == [rm["access"] for rm in rms]
            sets = sum(g[0] in (device.ACCESS_SET_PRIVATE, device.ACCESS_SET_PUBLIC) for g in got)
            # the first three set, the next three stand in fixed rooms, and past those whoever stands in a room just set waits
            assert sets == min(k, 3) and sum(g[0] == device.ACCESS_DEFERRED for g in got) == sum(1 for j in actors[6:] if j % 6 >= 3)
        assert state == list(accesses)                                  # periodic


@pytest.mark.gpu
def test_devpath_access_prints_one_line_with_the_parts_and_the_cpu(built):
    j = child_run.run_devpath("devpath --access", 300, "--access", "1,8",
                              "--reps", "3", "--warmup", "1", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and not {"plan", "roster", "look", "relay", "who", "rooms", "go"} & set(j)
    assert j["access_kernels"][:2] == list(device.ACCESS_KERNELS) and j["access_end_to_end_covers"] and j["access_plan_covers"]
    assert j["access_cpu_us_covers"]
    cs = j["access"]
    assert [(c["colour"], c["k"]) for c in cs] == [(colour, k) for colour in devpath.COLOURS for k in (1, 8)]
    for c in cs:
        assert c["n"] == 1000 and c["rooms"] == 6 and c["set"] + c["refused"] + c["deferred"] == c["k"] and c["set"] == min(c["k"], 3)
        assert c["public_set"] == c["set"] and c["public_set"] + c["public_refused"] + c["public_deferred"] == c["k"]
        assert c["lines"] == c["set"] + c["k"] - c["deferred"]
        for step in (c, c["public"]):
            assert 0 < step["kernels_us"]["median"] <= step["end_to_end_us"]["median"] <= step["python_us"]["median"]
            # the events and the room table the call before changed, 1,072 bytes a room; never the 5 bytes a slot of the table
            assert 6 * 1072 < step["h2d_bytes"] < 6 * 1072 + 4096
        assert c["cpu_us"]["median"] > 0 and c["end_to_end_over_cpu"] > 0 and c["plan"]["end_to_end_us"]["median"] > 0
        assert c["plan"]["h2d_bytes"] < 4096 and all(v > 0 for v in c["access_over_plan"].values())
    print("\n[devpath --access]", json.dumps(cs)[:3000])
