"""``python -m nuts333_amd.devpath --who K[,K...]``: who_many timed beside the CPU composing and transducing who()'s strings.

Host tier: the option rejects what ``--per-call`` rejects; with no GPU visible the command still exits 2 and measures
nothing; the strings the CPU composes are what the model of ``who()`` composes for the roster the command builds.
GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``, prints one line whose
``who`` section has a case per colour and K with the device's times and the CPU's.  No time is a pass condition.
"""
from __future__ import annotations

import json

import pytest

import child_run
from device_look_child import new_room
from device_who_child import colour_com_count, who, who_user
from nuts333_amd import device, devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "10,-3", "x", "1,x", "", "1,,2", "2.5"])
def test_who_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--who", value])
    assert e.value.code == 2
    assert "argument --who:" in capsys.readouterr().err


def test_who_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "who_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--who", "1,8"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_who_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.who_cases([1], 1, 0, {})


def test_the_strings_handed_to_the_cpu_are_the_models():
    n, names = 1000, devpath.LOOK_ROOMS
    rooms = [new_room(name) for name in names]
    users = {j: who_user(j, name=b"User%d" % j, room=j % len(names), desc=b"is user %d" % j, last_login=60 * j) for j in range(n)}
    for slot in (0, 1, 4, 63, 999):
        assert devpath.who_strings(n, slot) == who(users, rooms, slot, devpath.WHO_NOW, devpath.WHO_DATE)
    assert len(devpath.who_strings(n, 0)) == 3 + n and len(devpath.who_strings(0, 0)) == 3
    for s in (b"~FR", b"~FBK", b"~OLI", b"~FBBM", b"~~FR", b"~", b"~F", b"  U ~FBBM~FBBT~RS"):
        assert devpath.colour_com_count(s) == colour_com_count(s)


@pytest.mark.gpu
def test_devpath_who_prints_one_line_with_both_sides(built):
    j = child_run.run_devpath("devpath --who", 300, "--who", "1,8", "--reps", "3", "--warmup", "1", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and not {"plan", "roster", "per_call", "review", "speak", "input", "tell", "look", "relay"} & set(j)
    assert j["who_kernels"] == ["nuts_roster_who", "nuts_roster_who_shown", "nuts_roster_speak_plan"] and j["who_end_to_end_covers"]
    assert j["who_kernels"][:2] == list(device.WHO_KERNELS) and "composing who()'s strings" in j["who_cpu_us_covers"]
    wh = j["who"]
    assert [(c["colour"], c["k"]) for c in wh] == [(colour, k) for colour in devpath.COLOURS for k in (1, 8)]
    for c in wh:
        assert c["n"] == 1000 and c["lines"] == 1000
        assert c["writes"] >= 1003 * c["k"] and c["bytes_out"] > 0
        assert 0 < c["kernels_us"]["median"] <= c["end_to_end_us"]["median"] <= c["python_us"]["median"]
        assert c["cpu_us"]["median"] > 0 and c["end_to_end_over_cpu"] > 0
        assert c["h2d_bytes"] > 0 and c["d2h_bytes"] > 0
    by_k = {k: {c["d2h_bytes"] for c in wh if c["k"] == k} for k in (1, 8)}
    assert all(len(v) == 1 for v in by_k.values()) and min(by_k[1]) < min(by_k[8])      # the bitmaps: a row per looker
    print("\n[devpath --who]", json.dumps(wh)[:3000])
