"""``python -m nuts333_amd.devpath --look K[,K...]``: look_many timed beside the CPU's transducer over look()'s strings.

Host tier: the option rejects what ``--per-call`` rejects; with no GPU visible the command still exits 2 and measures
nothing; the strings it hands the CPU's transducer are what the model of ``look()`` composes for the roster it builds.
GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``, prints one line whose
``look`` section has a case per colour and K with the device's times, the CPU's, and what the CPU's leave out.  No time
is a pass condition.
"""
from __future__ import annotations

import json

import pytest

import child_run
from device_look_child import look, look_user, new_room
from nuts333_amd import device, devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "10,-3", "x", "1,x", "", "1,,2", "2.5"])
def test_look_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--look", value])
    assert e.value.code == 2
    assert "argument --look:" in capsys.readouterr().err


def test_look_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "look_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--look", "1,8"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_look_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.look_cases([1], 1, 0, {})


def test_the_strings_handed_to_the_cpu_are_the_models():
    n, names = 1000, devpath.LOOK_ROOMS
    rooms = [new_room(name, links=[(i + 1) % len(names)], mesg_cnt=i, topic=b"the topic of room %d" % i,
                      desc=b"The %s.\nA second line of description.\n" % name) for i, name in enumerate(names)]
    users = {j: look_user(j, name=b"User%d" % j, room=j % len(names), desc=b"is user %d" % j) for j in range(n)}
    for slot in (0, 1, 4, 63, 999):
        assert devpath.look_strings(n, slot) == look(users, rooms, slot)
        assert len(devpath.look_strings(n, slot)) == 7 + 199
    assert devpath.look_strings(3, 1)[3] == b"~FTYou are all alone here.\n" and len(devpath.look_strings(3, 1)) == 7


@pytest.mark.gpu
def test_devpath_look_prints_one_line_with_both_sides(built):
    j = child_run.run_devpath("devpath --look", 600, "--look", "1,8,64", "--reps", "5", "--warmup", "1", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and not {"plan", "roster", "per_call", "review", "speak", "input", "tell"} & set(j)
    assert j["look_kernels"] == ["nuts_roster_look", "nuts_roster_speak_plan"] and j["look_end_to_end_covers"]
    assert set(j["look_kernels"]) <= set(device.KERNELS) and "leaves the CPU's composing out" in j["look_cpu_us_covers"]
    lk = j["look"]
    assert [(c["colour"], c["k"]) for c in lk] == [(colour, k) for colour in devpath.COLOURS for k in (1, 8, 64)]
    for c in lk:
        assert c["n"] == 1000 and c["rooms"] == min(c["k"], 5) and c["members"] == 199 * c["k"]
        assert c["writes"] >= (7 + 199) * c["k"] and c["bytes_out"] > 0
        assert 0 < c["kernels_us"]["median"] <= c["end_to_end_us"]["median"] <= c["python_us"]["median"]
        assert c["cpu_us"]["median"] > 0 and c["end_to_end_over_cpu"] > 0
        assert c["h2d_bytes"] > 0 and c["d2h_bytes"] > 0
    by_k = {k: {c["d2h_bytes"] for c in lk if c["k"] == k} for k in (1, 8, 64)}
    assert all(len(v) == 1 for v in by_k.values())                      # with the lookers and their rooms alone
    assert min(by_k[1]) < min(by_k[8]) < min(by_k[64])
    print("\n[devpath --look]", json.dumps(lk)[:3000])
