"""``python -m nuts333_amd.devpath --speak K[,K...]``: speak_many timed beside plan_many of the same lines composed
beforehand, and beside the CPU composing them.

Host tier: the option rejects what ``--per-call`` rejects; with no GPU visible the command still exits 2 and measures
nothing; the events it times compose the texts the other sections time.  GPU tier: the command, at a small repetition
count, in one short-lived child under ``timeout``, prints one line whose ``speak`` section has a case per colour and K
with both sides' times and a download that grows with K alone.  No time is a pass condition.
"""
from __future__ import annotations

import ctypes
import json

import pytest

import child_run
from device_speak_child import model
from nuts333_amd import device, devpath, nuts_path


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "10,-3", "x", "1,x", "", "1,,2", "2.5"])
def test_speak_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--speak", value])
    assert e.value.code == 2
    assert "argument --speak:" in capsys.readouterr().err


def test_speak_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "speak_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--speak", "1,10"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_speak_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.speak_cases([1], 1, 0, {"format_line_once_ns": 1.0})


def test_the_timed_events_compose_the_say_texts():
    speaker = {"slot": 0, "room": 0, "name": b"Uaaa", "vis": 1, "muzzled": 0, "command_mode": 0}
    events = devpath.speak_events(12)
    assert [model(speaker, com, inpstr, wc, True)["line"] for _, com, inpstr, wc in events] == devpath.line_texts("say", 12)
    words = ctypes.create_string_buffer(10 * 41)
    assert all(slot == 0 and com == device.COM_SAY and wc == nuts_path.lib().np_wordfind(inpstr, words)
               for slot, com, inpstr, wc in events)
    cpu = devpath.speak_cpu_us(events, 3, 1)
    assert 0 < cpu["p10"] <= cpu["median"] <= cpu["p90"]


@pytest.mark.gpu
def test_devpath_speak_prints_one_line_with_both_sides(built):
    j = child_run.run_devpath("devpath --speak", 600, "--speak", "1,8,64",
                              "--reps", "10", "--warmup", "2", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and not {"plan", "roster", "per_call", "review"} & set(j)     # the other sections as they were
    assert j["speak_kernels"] == ["nuts_roster_speak", "nuts_roster_speak_plan"] and j["speak_end_to_end_covers"]
    assert set(j["speak_kernels"]) <= set(device.KERNELS)
    sp = j["speak"]
    assert [(c["colour"], c["k"]) for c in sp] == [(colour, k) for colour in devpath.COLOURS for k in (1, 8, 64)]
    for c in sp:
        assert c["n"] == 1000 and c["recipients"] == c["k"] * 999
        for side in (c, c["plan_many_of_the_composed_lines"]):
            assert 0 < side["kernels_us"]["median"] <= side["end_to_end_us"]["median"] <= side["python_us"]["median"]
            assert side["h2d_bytes"] > 0 and side["d2h_bytes"] > 0
        assert c["d2h_bytes"] > c["plan_many_of_the_composed_lines"]["d2h_bytes"]             # two plans and the texts
        assert set(c["composing_adds_us"]) == {"kernels_us", "end_to_end_us", "python_us"}
        assert c["cpu_us"]["median"] > 0 and c["cpu_derived_us"] > 0
    by_k = {k: {c["d2h_bytes"] for c in sp if c["k"] == k} for k in (1, 8, 64)}
    assert all(len(v) == 1 for v in by_k.values())                                          # with K alone
    assert min(by_k[1]) < min(by_k[8]) < min(by_k[64])
    print("\n[devpath --speak]", json.dumps(sp)[:3000])
