"""``python -m nuts333_amd.devpath --act K[,K...]``: act_many timed beside plan_many and look_many of the same lines and users
and beside the CPU.

Host tier: the option rejects what ``--per-call`` rejects; with no GPU visible the command still exits 2 and measures
nothing; the events the command submits -- K ``.wake`` events, K ``.move`` events there and K back, by K WIZ actors -- are
answered by the model of tests/device_act_child.py as the command's own model expects, text by text, and the moves back
end where the moves there began.
GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``, prints one line whose
``act`` section has a case per colour and K with the device's times, the parts' and the CPU's.  No time is a pass
condition but their order: the kernels within the call, the call within the Python call.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import child_run
from device_act_child import KINDS, act_call, act_user
from device_rooms_child import list_room
from nuts333_amd import device, devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "x", "", "1,,2", "2.5"])
def test_act_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--act", value])
    assert e.value.code == 2
    assert "argument --act:" in capsys.readouterr().err


def test_act_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "act_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--act", "1,8"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_act_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.act_cases([1], 1, 0, {})


def test_the_calls_the_command_submits_are_answered_as_it_expects():
    n, half = 1000, devpath.ACT_HALF
    names, accesses = devpath.ROOMS_LISTS["6"]
    home = np.arange(n) % 6
    for k in (1, 8, 64):
        rms = [list_room(name, access=access, links=list(links)) for name, access, links in zip(names, accesses, devpath.GO_LINKS)]
        users = {j: act_user(j, name=b"User%d" % j, room=j % 6, level=2 if j < half else 1) for j in range(n)}
        actors = [j % half for j in range(k)]
        target = lambda j: half + j % half
        wake = [(j, device.COM_WAKE, b"user%d" % target(j), 2) for j in actors]
        there = [(j, device.COM_MOVE, b"user%d %s" % (target(j), names[(int(home[target(j)]) + 1) % 6]), 3) for j in actors]
        back = [(j, device.COM_MOVE, b"user%d %s" % (target(j), names[int(home[target(j)])]), 3) for j in actors]
        room_of = home.copy()
        for events in (wake, there, back):
            want = devpath.act_model(room_of, events)
            call = act_call(users, rms, [], events, 3, 2)
            assert [e["outcome"] for e in call["events"]] == [w[0] for w in want]
            for e, w in zip(call["events"], want):
                assert {kind: e[kind] for kind in KINDS if e[kind] is not None} == w[3]
                if w[0] != device.ACT_DEFERRED:
                    assert (e["target_slot"], e["target_room"]) == w[1:3]
            if events is wake:
                assert [w[0] for w in want] == [device.ACT_WOKEN] * k            # a wake changes nothing: every one is answered
            else:
                assert sum(w[0] == device.ACT_MOVED for w in want) == min(k, 2)  # six rooms take two moves a call
        assert np.array_equal(room_of, home) and [users[j]["room"] for j in range(n)] == home.tolist()      # periodic


@pytest.mark.gpu
def test_devpath_act_prints_one_line_with_the_parts_and_the_cpu(built):
    j = child_run.run_devpath("devpath --act", 300, "--act", "1,8", "--reps", "3", "--warmup", "1", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and not {"plan", "roster", "look", "relay", "who", "rooms", "go", "access", "clone", "set"} & set(j)
    assert j["act_kernels"][:2] == list(device.ACT_KERNELS) and j["act_end_to_end_covers"] and j["act_parts_covers"]
    assert j["act_cpu_us_covers"]
    cs = j["act"]
    assert [(c["colour"], c["k"]) for c in cs] == [(colour, k) for colour in devpath.COLOURS for k in (1, 8)]
    for c in cs:
        assert c["n"] == 1000 and c["rooms"] == 6 and c["woken"] == c["k"] and c["wake_lines"] == 2 * c["k"]
        assert c["moved"] == c["back_moved"] == min(c["k"], 2) == c["k"] - c["deferred"] - c["already"] and c["move_lines"] == 5 * c["moved"]
        for step in (c["wake"], c["wake"]["parts"], c["move"], c["move"]["parts"], c["back"]):
            assert 0 < step["kernels_us"]["median"] <= step["end_to_end_us"]["median"] <= step["python_us"]["median"]
        # the events alone in a wake call; a call that moves carries the table its last look did not have to, in the look
        assert c["wake"]["h2d_bytes"] < 4096 and 5000 < c["move"]["h2d_bytes"] < 5000 + 8192
        for part in ("wake", "move"):
            assert c[part]["cpu_us"]["median"] > 0 and all(v > 0 for v in c[part]["over_parts"].values())
            assert all(lo <= c[part]["over_parts"][f] <= hi for f, (lo, hi) in c[part]["over_parts_p10_p90"].items())
    print("\n[devpath --act]", json.dumps(cs)[:3000])
