"""``python -m nuts333_amd.devpath --rooms K[,K...]``: rooms_many timed beside the CPU composing and transducing rooms()'s
strings.

Host tier: the option rejects what ``--per-call`` rejects; with no GPU visible the command still exits 2 and measures
nothing; the strings the CPU composes are what the model of ``rooms()`` composes for the rosters the command builds.
GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``, prints one line whose
``rooms`` section has a case per room list, colour, kind and K with the device's times and the CPU's.  No time is a pass
condition.
"""
from __future__ import annotations

import json

import pytest

import child_run
from device_look_child import look_user
from device_rooms_child import HEAD_LINKS, HEAD_TOPICS, list_room, rooms
from nuts333_amd import device, devpath
from nuts333_amd.provision import SIX_ROOMS


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "10,-3", "x", "1,x", "", "1,,2", "2.5"])
def test_rooms_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--rooms", value])
    assert e.value.code == 2
    assert "argument --rooms:" in capsys.readouterr().err


def test_rooms_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "rooms_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--rooms", "1,8"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_rooms_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.rooms_cases([1], 1, 0, {})


def test_the_strings_handed_to_the_cpu_are_the_models():
    n = 1000
    assert devpath.ROOMS_HEADS == {True: HEAD_TOPICS, False: HEAD_LINKS}
    assert [r.name.encode() for r in SIX_ROOMS] == devpath.ROOMS_LISTS["6"][0] and len(devpath.ROOMS_LISTS["1024"][0]) == device.MAX_LOOK_ROOMS
    for which, (names, accesses) in devpath.ROOMS_LISTS.items():
        nr = len(names)
        rms = [list_room(name, access=access, mesg_cnt=i, topic=b"the topic of room %d" % i, inlink=i % 3 == 0,
                         netlink=(b"service%d" % i, False, i % 3) if i % 5 == 0 else None)
               for i, (name, access) in enumerate(zip(names, accesses))]
        users = {j: look_user(j, name=b"User%d" % j, room=j % nr) for j in range(n)}
        for topics in (True, False):
            assert devpath.rooms_strings(n, which, topics) == rooms(users, rms, topics), (which, topics)
            assert len(devpath.rooms_strings(n, which, topics)) == 2 + nr


@pytest.mark.gpu
def test_devpath_rooms_prints_one_line_with_both_sides(built):
    j = child_run.run_devpath("devpath --rooms", 300, "--rooms", "1,8", "--reps", "3", "--warmup", "1", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and not {"plan", "roster", "per_call", "review", "speak", "input", "tell", "look", "relay", "who"} & set(j)
    assert j["rooms_kernels"] == ["nuts_roster_rooms_count", "nuts_roster_rooms_lines", "nuts_roster_speak_plan"] and j["rooms_end_to_end_covers"]
    assert j["rooms_kernels"][:2] == list(device.ROOMS_KERNELS) and "composing rooms()'s strings" in j["rooms_cpu_us_covers"]
    rs = j["rooms"]
    assert [(c["rooms"], c["colour"], c["kind"], c["k"]) for c in rs] == [(nr, colour, kind, k) for nr in (6, 1024) for colour in devpath.COLOURS
                                                                          for kind in ("rmst", "rmsn") for k in (1, 8)]
    for c in rs:
        assert c["n"] == 1000 and c["writes"] >= (2 + c["rooms"]) * c["k"] and c["bytes_out"] > 0
        assert 0 < c["kernels_us"]["median"] <= c["end_to_end_us"]["median"] <= c["python_us"]["median"]
        assert c["cpu_us"]["median"] > 0 and c["end_to_end_over_cpu"] > 0
        assert c["h2d_bytes"] == 256 + 4 and c["d2h_bytes"] > 0          # clean mirrors: the lookers alone
    # the download is at the bound size: it depends on the room count alone, not on K or on the kind
    assert all(len({c["d2h_bytes"] for c in rs if c["rooms"] == nr}) == 1 for nr in (6, 1024))
    print("\n[devpath --rooms]", json.dumps(rs)[:3000])
