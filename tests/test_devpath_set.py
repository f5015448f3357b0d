"""``python -m nuts333_amd.devpath --set K[,K...]``: set_many timed beside speak_many of the same bodies and beside the CPU.

Host tier: the option rejects what ``--per-call`` rejects; with no GPU visible the command still exits 2 and measures
nothing; the events the command submits -- K ``.ignall`` events and K ``.desc <text>`` events by K actors -- are answered
by the model of tests/device_set_child.py as the command expects, and two ``.ignall`` calls end where they began.
GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``, prints one line whose
``set`` section has a case per colour and K with the device's times, ``speak_many``'s and the CPU's.  No time is a pass
condition but their order: the kernels within the call, the call within the Python call.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import child_run
from device_rooms_child import list_room
from device_set_child import set_call, set_user
from nuts333_amd import device, devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "x", "", "1,,2", "2.5"])
def test_set_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--set", value])
    assert e.value.code == 2
    assert "argument --set:" in capsys.readouterr().err


def test_set_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "set_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--set", "1,8"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_set_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.set_cases([1], 1, 0, {})


def test_the_calls_the_command_submits_are_answered_as_it_expects():
    n = 1000
    names, accesses = devpath.ROOMS_LISTS["6"]
    room_of = np.arange(n) % 6
    for k in (1, 8, 64):
        rms = [list_room(name, access=access, links=list(links)) for name, access, links in zip(names, accesses, devpath.GO_LINKS)]
        users = {j: set_user(j, name=b"User%d" % j, room=j % 6, level=1) for j in range(n)}
        ignalls, descs, says = devpath.set_events(k)
        actors = list(range(k))
        assert [ev[0] for ev in ignalls] == [ev[0] for ev in descs] == [ev[0] for ev in says] == actors
        assert [ev[2] for ev in descs] == [ev[2] for ev in says] and all(0 < len(ev[2]) <= device.USER_DESC_LEN for ev in descs)
        for on in (True, False):
            call = set_call(users, rms, ignalls)
            assert [e["outcome"] for e in call["events"]] == devpath.set_model(room_of, actors, on)
            assert sum(e["outcome"] != device.SET_DEFERRED for e in call["events"]) == min(k, 6)
            line = b"User%d is now ignoring everyone.\n" if on else b"User%d is listening again.\n"
            assert all(e["here"] == line % j for j, e in enumerate(call["events"]) if e["outcome"] != device.SET_DEFERRED)
        assert not any(u["ignall"] for u in users.values())             # periodic
        call = set_call(users, rms, descs)
        assert [e["outcome"] for e in call["events"]] == [device.SET_DESC_SET] * k
        assert all(e["reply"] == b"Description set.\n" and e["here"] is None for e in call["events"])
        assert [users[j]["desc"] for j in actors] == [ev[2] for ev in descs]


@pytest.mark.gpu
def test_devpath_set_prints_one_line_with_the_parts_and_the_cpu(built):
    j = child_run.run_devpath("devpath --set", 300, "--set", "1,8", "--reps", "3", "--warmup", "1", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and not {"plan", "roster", "look", "relay", "who", "rooms", "go", "access", "clone"} & set(j)
    assert j["set_kernels"][:2] == list(device.SET_KERNELS) and j["set_end_to_end_covers"] and j["set_speak_covers"]
    assert j["set_cpu_us_covers"]
    cs = j["set"]
    assert [(c["colour"], c["k"]) for c in cs] == [(colour, k) for colour in devpath.COLOURS for k in (1, 8)]
    for c in cs:
        assert c["n"] == 1000 and c["rooms"] == 6 and c["toggled"] == min(c["k"], 6) == c["k"] - c["deferred"]
        for step in (c["ignall"], c["ignall"]["speak"], c["desc"], c["desc"]["speak"]):
            assert 0 < step["kernels_us"]["median"] <= step["end_to_end_us"]["median"] <= step["python_us"]["median"]
        # the events alone in the .ignall call: the table it changes, 5 bytes a slot, travels with the speak_many of its rounds;
        # the .desc call carries the descriptions its last call changed, 32 bytes a slot, and the speaker table behind them, 16
        assert c["ignall"]["h2d_bytes"] < 4096 and 5000 < c["ignall"]["speak"]["h2d_bytes"] < 5000 + 5120
        assert 48000 <= c["desc"]["h2d_bytes"] < 48000 + 4096 and c["desc"]["speak"]["h2d_bytes"] < 4096
        for part in ("ignall", "desc"):
            assert c[part]["cpu_us"]["median"] > 0 and all(v > 0 for v in c[part + "_over_speak"].values())
            assert all(lo <= c[part + "_over_speak"][f] <= hi for f, (lo, hi) in c[part + "_over_speak_p10_p90"].items())
    print("\n[devpath --set]", json.dumps(cs)[:3000])
